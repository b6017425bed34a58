// cooc_rescore.h — launch wrappers of cooc_rescore.hip (LLR rescoring: top-k heaps of rows of counts).
#pragma once

#include "cooc_device.h"

namespace cooc {

// LogLikelihood.logLikelihoodRatio (the rescorer's device scoring function) over n (k11, k12, k21, k22)
Status launch_llr(hipStream_t s, int64_t n, const int64_t *d_k4, double *d_out);

// The touched rows of a streaming window (touched, scal[0] of them) against the dense global rows G.
// scal: [0] touched rows, [2] rescorer observed (cumulative), [3] exact observed (cumulative).
Status launch_rescore(hipStream_t s, const int32_t *touched, const int64_t *scal, int32_t M, const uint32_t *G,
                      const int64_t *grs, bool exact, int32_t topk, int32_t max_rows, DevBuf &terms, int32_t *out_size,
                      int32_t *out_val, double *out_score);
// ... against the sparse global rows (n_items >= 40,320: struct GlobalSparse, cooc_device.h)
Status launch_rescore_sparse(hipStream_t s, const int32_t *touched, const int64_t *scal, int32_t M, const GlobalSparse &g,
                             const int64_t *grs, bool exact, int32_t topk, int32_t max_rows, DevBuf &terms,
                             int32_t *out_size, int32_t *out_val, double *out_score);

// LLR top-k of every row of a batch result (padded CSR) -- the C5 stage over one window.
// obs3 (device int64[3]) receives the rescorer's observed, the exact observed and n_items; terms is
// scratch for the per-column LLR terms (32 B per item).
Status launch_rescore_batch(hipStream_t s, int32_t M, const int64_t *row_base, const int32_t *row_nnz,
                            const int32_t *col, const uint32_t *cnt, const uint32_t *dense, const int64_t *rowsum,
                            bool exact, int32_t topk,
                            int64_t *obs3, DevBuf &terms, int32_t *out_size, int32_t *out_val, double *out_score,
                            const int32_t *rank_of = nullptr, bool unordered = true, int64_t nnz = -1,
                            bool whole_log = false);

}  // namespace cooc
