"""A numpy model of the batch planner's plan (cooc_count.hip: k_batch_users, k_batch_plan, k_batch_chunks and the
batches and walker ranges of k_acc_batch), written from the formulas and not from what the library reports:

  B    = max(1, min(n_cu, n // 4096 + 1))          partition blocks of the hist / scatter passes
  db   = min(1024, (160 * 1024 - 1536 - 4 * ((M + 2) & ~1) - 4) // 12)   descriptors per batch
  lbar = sum over contributions of the padded length of the list they walk / n   (float64, as in k_batch_plan)
  nch  = min(c, max(1, ceil(c * lbar / 2^22)))     chunks of a row of c contributions
  chunk j of a row = contributions [cnt * j // nch, cnt * (j + 1) // nch) of it

One window over empty histories (old is None): every position of a list contributes the whole list.  Streaming
windows: user j's list is its history after the window, old[j] its length before; a new position (index >= old[j])
contributes the whole list, an old position the new part (its own padded segment, no self term).

The group totals of a row's batches (8 ids per 16-B group) are those of the row's contributions in position order.
The library's scatter orders a row's descriptors by partition block and, inside a block, by the order its LDS
atomics land in, so for a row of several batches the totals of the single batches are nominal; their sum over the
row, and the totals of a row of one batch, do not depend on the order.
"""
import numpy as np

K_WALKERS = {"dense": 64, "csr": 128}     # k_acc_batch<4, 16, true> and <4, 8, false>: 1024 / S walkers
STEP_GROUPS = {"dense": 64, "csr": 32}    # one walker step: S lanes x 4 loads
CHUNK_WORK = 1 << 22
FILL_THREAD = 2048


def pad8(x):
    return (np.asarray(x, np.int64) + 7) & ~np.int64(7)


def batch_db(M):
    return min(1024, (160 * 1024 - 1536 - 4 * ((M + 2) & ~1) - 4) // 12)


class BatchPlan:
    def __init__(self, user_ptr, items, M, n_cu, old=None):
        up = np.asarray(user_ptr, np.int64)
        it = np.asarray(items, np.int64)
        n = int(up[-1]) if len(up) else 0
        assert len(it) == n
        lens = np.diff(up)
        o = np.zeros(len(lens), np.int64) if old is None else np.asarray(old, np.int64)
        assert np.all(o >= 0) and np.all(o <= lens)
        self.M, self.n, self.n_cu = M, n, n_cu
        self.B = max(1, min(n_cu, n // 4096 + 1))
        self.db = batch_db(M)
        self.max_len = int(lens.max()) if len(lens) else 0
        self.n_long = int(np.sum(lens > FILL_THREAD))
        pl = pad8(lens)
        pn = np.where(o > 0, pad8(lens - o), 0)
        self.sum_lpl = int(np.sum((lens - o) * pl + o * pn))
        self.sum_l2 = int(np.sum((lens - o) * lens + o * (lens - o)))
        self.lbar = np.float64(self.sum_lpl) / np.float64(n) if n > 0 else np.float64(0.0)
        self.c = np.bincount(it, minlength=M).astype(np.int64)
        w = self.c.astype(np.float64) * self.lbar
        nch = np.minimum(self.c.astype(np.float64), np.maximum(1.0, np.ceil(w / np.float64(CHUNK_WORK))))
        self.nch = np.where(self.c > 0, nch, 0).astype(np.int64)
        self.n_chunks = int(self.nch.sum())
        self.n_split = int(np.sum(self.nch > 1))
        # the contributions in row order (positions ascending inside a row) and the length each one walks
        user = np.repeat(np.arange(len(lens)), lens)
        pos = np.arange(n, dtype=np.int64) - np.repeat(up[:-1], lens)
        self.is_old = pos < o[user]
        self.walk_len = np.where(self.is_old, (lens - o)[user], lens[user])
        self._order = np.argsort(it, kind="stable")
        self.row_ptr = np.concatenate([[0], np.cumsum(self.c)]).astype(np.int64)
        self._user, self._up = user, up

    def expected(self, dense):
        """What cooc_last_batch_plan reports for this run."""
        return (self.B, self.db, self.n_chunks, self.n_split, int(bool(dense)), self.max_len, self.n_long, 0)

    def block_bounds(self):
        """The interaction ranges' inner boundaries n * b // B of the partition blocks."""
        return [self.n * b // self.B for b in range(1, self.B)]

    def chunks(self, a):
        """Row a's chunks as contribution ranges relative to the row's first contribution."""
        cnt, nch = int(self.c[a]), int(self.nch[a])
        return [(cnt * j // nch, cnt * (j + 1) // nch) for j in range(nch)]

    def row_positions(self, a):
        """The log positions of row a's contributions, in the nominal descriptor order."""
        return self._order[self.row_ptr[a]:self.row_ptr[a + 1]]

    def row_groups(self, a):
        """Groups (16-B loads) of every contribution of row a, in the nominal order."""
        return (self.walk_len[self.row_positions(a)] + 7) >> 3

    def row_old(self, a):
        return self.is_old[self.row_positions(a)]

    def row_users(self, a):
        return self._user[self.row_positions(a)]

    def batches(self, a):
        """Per chunk of row a, per batch: (descriptors, group total)."""
        g = self.row_groups(a)
        out = []
        for lo, hi in self.chunks(a):
            out.append([(min(self.db, hi - b0), int(g[b0:min(hi, b0 + self.db)].sum()))
                        for b0 in range(lo, hi, self.db)])
        return out

    def block_of(self, p):
        """Partition block of log position p (block b covers [n b // B, n (b + 1) // B))."""
        return np.searchsorted(np.asarray(self.block_bounds(), np.int64), np.asarray(p, np.int64), side="right")


def walker_ranges(total, layout):
    """[lo, hi) group range of every walker of a batch of `total` groups."""
    kw = K_WALKERS[layout]
    q = np.arange(kw + 1, dtype=np.int64)
    e = total * q // kw
    return e[:-1], e[1:]


def walker_steps(total, layout):
    """Steps of the busiest walker (0: no group at all)."""
    lo, hi = walker_ranges(total, layout)
    return int(-(-int((hi - lo).max()) // STEP_GROUPS[layout]))


def wave_ranges(M, align):
    """The 16 waves' column ranges of the compactions: align = 256 (compact_row_ranges4) or 64 (compact_row_ranges,
    k_pack_dense); empty ranges left out."""
    per = ((M + 15) // 16 + align - 1) & ~(align - 1)
    out = []
    for w in range(16):
        lo = min(M, w * per)
        hi = min(M, lo + per)
        if lo < hi:
            out.append((lo, hi))
    return out
