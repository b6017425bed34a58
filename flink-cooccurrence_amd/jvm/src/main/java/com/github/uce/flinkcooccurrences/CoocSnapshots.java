package com.github.uce.flinkcooccurrences;

import java.nio.ByteBuffer;
import java.nio.ByteOrder;
import java.util.Map;
import java.util.TreeMap;
import org.apache.flink.api.common.state.ListState;
import org.apache.flink.api.common.state.ListStateDescriptor;
import org.apache.flink.api.java.tuple.Tuple1;
import org.apache.flink.runtime.state.KeyGroupRangeAssignment;
import org.apache.flink.runtime.state.StateInitializationContext;

/**
 * Moves a handle's streaming state through Flink's operator state: what was windowState and userHistoryState in
 * the reference (NonSampled...java:73-77) and itemRows / globalItemRowSums in its rescorer lives in the handle, so
 * a checkpoint saves the handle's snapshot blob instead.
 *
 * <p>The blobs are union list state: on a restore every subtask receives the blobs of ALL subtasks of the job
 * that wrote the checkpoint.  snapshotState: {@link #write} after the operator handed its buffered records to
 * the handle (CoocNative.processElements: they join the handle's buffered windows, which the blob carries).  A
 * blob goes out as list elements of at most {@link #MAX_RANGE} payload bytes, a blob being possibly larger than
 * one Java array.  Every element starts with {@link #PREFIX} bytes: the Flink subtask index and parallelism that
 * wrote it, the blob's length, the range's offset, and the library's (rank, world) of the handle.  The ranges
 * find their blob again by the SUBTASK INDEX, whatever order the union arrives in: a handle that joined no
 * communicator writes (rank 0, world 1) on every subtask, so the library's rank does not tell the blobs apart.
 *
 * <p>initializeState runs before open(), where the handle is created (and, where the operator does so, joins its
 * communicator), so {@link #read} only keeps the ranges and open() installs them with {@link #install}:
 * <ul>
 *   <li>at the parallelism that wrote the checkpoint a subtask restores its own blob (cooc_restore_finish: the
 *       same (rank, world) and user sharding), with or without a communicator;
 *   <li>at another parallelism, and only when the old handles had joined a communicator of the job's parallelism
 *       (every blob's (rank, world) is its (subtask, parallelism)), it hands all blobs to the library
 *       (cooc_restore_finish_parts) with a bitmap of the users it keeps, filled from Flink's own key-group
 *       assignment of each user id; the library installs the global rows a mod p == subtask, every item's row
 *       sum, the kept users' histories and buffered records, and the job's totals.  User ids must be
 *       non-negative for that (a bitmap has no bit for a negative id);
 *   <li>at another parallelism with handles that had joined no communicator the restore is refused: such a
 *       handle holds partial rows of every item for its own users, not the rows a mod p, so the blobs cannot be
 *       repartitioned.  Restart at the parallelism that wrote the checkpoint.
 * </ul>
 */
final class CoocSnapshots {

  /** Payload bytes per list element: the largest array a JVM allocates reliably, less the prefix. */
  static final int PREFIX = 32;
  static final int MAX_RANGE = Integer.MAX_VALUE - 8 - PREFIX;

  static final ListStateDescriptor<byte[]> DESCRIPTOR = new ListStateDescriptor<>("cooc-snapshot-blobs", byte[].class);

  /** A blob read back from a checkpoint: its list elements (prefix, then the range's bytes) by offset. */
  static final class Blob {
    int subtask;      // the Flink subtask that wrote it ...
    int parallelism;  // ... in a job of this parallelism
    int rank;         // the library's (rank, world) of its handle: (0, 1) without a communicator
    int world;
    long bytes;
    final TreeMap<Long, byte[]> ranges = new TreeMap<>();  // offset -> element (prefix + payload)
  }

  /** The blobs of a restored checkpoint: all subtasks' of the job that wrote it, by subtask index. */
  static final class Restored {
    final TreeMap<Integer, Blob> parts = new TreeMap<>();
  }

  private CoocSnapshots() {}

  /** The union list state that carries the blobs; called from initializeState. */
  static ListState<byte[]> state(StateInitializationContext context) throws Exception {
    return context.getOperatorStateStore().getUnionListState(DESCRIPTOR);
  }

  /**
   * The handle's state into the checkpoint (prepare, ranged copies, release); called from snapshotState with the
   * subtask's index and the job's parallelism.
   */
  static void write(long handle, ListState<byte[]> state, int subtask, int parallelism) throws Exception {
    final long[] info = new long[10];
    CoocNative.snapshotPrepare(handle, info);
    try {
      state.clear();
      final long bytes = info[0];
      for (long offset = 0; offset < bytes; ) {
        final int n = (int) Math.min(bytes - offset, MAX_RANGE);
        final byte[] payload = new byte[n];
        CoocNative.snapshotCopy(handle, offset, n, payload);
        final byte[] element = new byte[PREFIX + n];
        ByteBuffer.wrap(element).order(ByteOrder.LITTLE_ENDIAN).putInt(subtask).putInt(parallelism)
            .putLong(bytes).putLong(offset).putInt((int) info[8]).putInt((int) info[9]);
        System.arraycopy(payload, 0, element, PREFIX, n);
        state.add(element);
        offset += n;
      }
    } finally {
      CoocNative.snapshotRelease(handle);
    }
  }

  /** The blobs of a restored checkpoint (null on a fresh start); called from initializeState. */
  static Restored read(StateInitializationContext context, ListState<byte[]> state) throws Exception {
    if (!context.isRestored()) {
      return null;
    }
    final Restored restored = new Restored();
    for (byte[] element : state.get()) {
      if (element.length < PREFIX) {
        throw new IllegalStateException("a snapshot list element shorter than its prefix");
      }
      final ByteBuffer head = ByteBuffer.wrap(element).order(ByteOrder.LITTLE_ENDIAN);
      final int subtask = head.getInt();
      final int parallelism = head.getInt();
      final long bytes = head.getLong();
      final long offset = head.getLong();
      final int rank = head.getInt();
      final int world = head.getInt();
      Blob blob = restored.parts.get(subtask);
      if (blob == null) {
        blob = new Blob();
        blob.subtask = subtask;
        blob.parallelism = parallelism;
        blob.rank = rank;
        blob.world = world;
        blob.bytes = bytes;
        restored.parts.put(subtask, blob);
      } else if (blob.parallelism != parallelism || blob.bytes != bytes || blob.rank != rank || blob.world != world) {
        throw new IllegalStateException("the ranges of subtask " + subtask + "'s snapshot blob disagree about it");
      }
      if (blob.ranges.put(offset, element) != null) {
        throw new IllegalStateException("subtask " + subtask + "'s snapshot blob holds offset " + offset + " twice");
      }
    }
    return restored.parts.isEmpty() ? null : restored;
  }

  /**
   * Installs a restored checkpoint into a freshly created handle; called from open() with the subtask's index,
   * the job's parallelism and its maximum parallelism (the key groups).
   */
  static void install(long handle, Restored restored, int subtask, int parallelism, int maxParallelism) {
    if (restored == null) {
      return;
    }
    final int oldParallelism = restored.parts.firstEntry().getValue().parallelism;
    boolean joined = true;  // every old handle had joined a communicator of the old job's parallelism
    for (Blob blob : restored.parts.values()) {
      if (blob.parallelism != oldParallelism) {
        throw new IllegalStateException("the checkpoint holds snapshot blobs of jobs of " + oldParallelism + " and "
            + blob.parallelism + " subtasks");
      }
      joined &= blob.world == oldParallelism && blob.rank == blob.subtask;
    }
    if (restored.parts.size() != oldParallelism || restored.parts.firstKey() != 0
        || restored.parts.lastKey() != oldParallelism - 1) {
      throw new IllegalStateException("the checkpoint holds " + restored.parts.size() + " snapshot blobs of a job of "
          + oldParallelism + " subtasks");
    }
    if (oldParallelism == parallelism) {  // the same parallelism and user sharding: this subtask's own blob
      final Blob blob = restored.parts.get(subtask);
      CoocNative.restoreBegin(handle, blob.bytes);
      for (Map.Entry<Long, byte[]> range : blob.ranges.entrySet()) {
        CoocNative.restoreWriteFrom(handle, range.getKey(), range.getValue(), PREFIX, range.getValue().length - PREFIX);
      }
      CoocNative.restoreFinish(handle, new long[10]);
    } else if (!joined) {
      throw new IllegalStateException("the checkpoint was written at parallelism " + oldParallelism + " by handles "
          + "without a communicator: each holds partial rows for its own users, which cannot be repartitioned; "
          + "restart at parallelism " + oldParallelism + " (this job runs at " + parallelism + ")");
    } else {  // rescaling: all blobs, and the users Flink's key groups send to this subtask
      final long[] sizes = new long[oldParallelism];
      long bound = 0;  // one past the largest user id of the checkpoint (at most 2^31)
      for (Blob blob : restored.parts.values()) {
        sizes[blob.subtask] = blob.bytes;
        bound = Math.max(bound, userIdBound(blob));
      }
      final long[] bits = new long[(int) ((bound + 63) / 64)];
      final Tuple1<Integer> key = new Tuple1<>();  // keyBy(0) keys a Tuple3 stream by Tuple1<Integer>
      for (long user = 0; user < bound; user++) {
        key.f0 = (int) user;
        if (KeyGroupRangeAssignment.assignKeyToParallelOperator(key, maxParallelism, parallelism) == subtask) {
          bits[(int) (user >> 6)] |= 1L << (user & 63);
        }
      }
      CoocNative.restoreBeginParts(handle, sizes);
      for (Blob blob : restored.parts.values()) {
        for (Map.Entry<Long, byte[]> range : blob.ranges.entrySet()) {
          CoocNative.restoreWritePart(handle, blob.subtask, range.getKey(), range.getValue(), PREFIX,
              range.getValue().length - PREFIX);
        }
      }
      CoocNative.restoreFinishParts(handle, CoocNative.ROUTE_BITMAP, bound, bits, new long[10]);
    }
    restored.parts.clear();
  }

  /** Byte {@code at} of a blob held in ranges. */
  private static int byteAt(Blob blob, long at) {
    final Map.Entry<Long, byte[]> range = blob.ranges.floorEntry(at);
    if (range == null || at - range.getKey() >= range.getValue().length - PREFIX) {
      throw new IllegalArgumentException("snapshot blob: a byte outside its ranges");
    }
    return range.getValue()[PREFIX + (int) (at - range.getKey())] & 0xff;
  }

  private static int intAt(Blob blob, long at) {
    return byteAt(blob, at) | byteAt(blob, at + 1) << 8 | byteAt(blob, at + 2) << 16 | byteAt(blob, at + 3) << 24;
  }

  private static long longAt(Blob blob, long at) {
    long v = 0;
    for (int i = 7; i >= 0; i--) {
      v = (v << 8) | byteAt(blob, at + i);
    }
    return v;
  }

  /**
   * One past the largest user id among a blob's histories (section 2) and buffered records (section 14): their
   * directory entries are at 64 + 40 (kind - 1), the offset at +8 and the element count at +24 (DESIGN.md §5c).
   * The library validates the blob; here a negative id only ends the restore early with a clear message.
   */
  private static long userIdBound(Blob blob) {
    long bound = 0;
    for (int kind : new int[] {2, 14}) {
      final long entry = 64 + 40L * (kind - 1);
      final long offset = longAt(blob, entry + 8);
      final long count = longAt(blob, entry + 24);
      if (offset < 0 || count < 0 || count > blob.bytes / 4 || offset > blob.bytes - 4 * count) {
        throw new IllegalArgumentException("snapshot blob: a section outside the blob");
      }
      for (long i = 0; i < count; i++) {
        final int user = intAt(blob, offset + 4 * i);
        if (user < 0) {
          throw new IllegalStateException("rescaling needs non-negative user ids; the checkpoint holds " + user);
        }
        bound = Math.max(bound, user + 1L);
      }
    }
    return bound;
  }
}
