package com.github.uce.flinkcooccurrences;

import java.io.DataInputStream;
import java.io.DataOutputStream;
import java.io.IOException;
import java.util.ArrayList;
import java.util.List;
import org.apache.flink.runtime.state.OperatorStateCheckpointOutputStream;
import org.apache.flink.runtime.state.StateInitializationContext;
import org.apache.flink.runtime.state.StatePartitionStreamProvider;
import org.apache.flink.runtime.state.StateSnapshotContext;

/**
 * Moves a handle's streaming state through Flink's raw operator state: what was windowState and
 * userHistoryState in the reference (NonSampled...java:73-77) and itemRows / globalItemRowSums in its rescorer
 * lives in the handle, so a checkpoint saves the handle's snapshot blob instead.
 *
 * <p>snapshotState: {@link #write} after the operator handed its buffered records to the handle
 * (CoocNative.processElements: they join the handle's buffered windows, which the blob carries).  The blob goes
 * out as one partition: its length, then ranges of at most {@link #MAX_RANGE} bytes, a blob being possibly larger
 * than one Java array.
 *
 * <p>initializeState runs before open(), where the handle is created (and, with p &gt; 1, joins its
 * communicator: a restore checks the blob's rank and world against it), so {@link #read} only keeps the ranges
 * and open() installs them with {@link #install}.  Restore is local: every subtask restores its own blob, which
 * needs the same parallelism and user sharding as the job that wrote it (no rescaling).
 */
final class CoocSnapshots {

  /** Bytes per range: the largest array a JVM allocates reliably. */
  static final int MAX_RANGE = Integer.MAX_VALUE - 8;

  /** A blob read back from a checkpoint, in ranges. */
  static final class Blob {
    long bytes;
    final List<byte[]> ranges = new ArrayList<>();
  }

  private CoocSnapshots() {}

  /** The handle's state into the checkpoint's raw operator state (prepare, ranged copies, release). */
  static void write(long handle, StateSnapshotContext context) throws IOException {
    final long[] info = new long[10];
    CoocNative.snapshotPrepare(handle, info);
    try {
      final OperatorStateCheckpointOutputStream raw = context.getRawOperatorStateOutput();
      raw.startNewPartition();
      final DataOutputStream out = new DataOutputStream(raw);
      final long bytes = info[0];
      out.writeLong(bytes);
      byte[] range = new byte[(int) Math.min(bytes, 1 << 26)];
      for (long offset = 0; offset < bytes; ) {
        final int n = (int) Math.min(bytes - offset, MAX_RANGE);
        if (n > range.length) {
          range = new byte[n];
        }
        CoocNative.snapshotCopy(handle, offset, n, range);
        out.write(range, 0, n);
        offset += n;
      }
      out.flush();
    } finally {
      CoocNative.snapshotRelease(handle);
    }
  }

  /** The blob of a restored checkpoint (null on a fresh start); called from initializeState. */
  static Blob read(StateInitializationContext context) throws IOException {
    if (!context.isRestored()) {
      return null;
    }
    Blob blob = null;
    for (StatePartitionStreamProvider partition : context.getRawOperatorStateInputs()) {
      if (blob != null) {
        throw new IllegalStateException("more than one snapshot blob for this subtask: rescaling is not supported");
      }
      final DataInputStream in = new DataInputStream(partition.getStream());
      blob = new Blob();
      blob.bytes = in.readLong();
      for (long offset = 0; offset < blob.bytes; ) {
        final byte[] range = new byte[(int) Math.min(blob.bytes - offset, MAX_RANGE)];
        in.readFully(range);
        blob.ranges.add(range);
        offset += range.length;
      }
    }
    return blob;
  }

  /** Installs a blob into a freshly created handle (begin, ranged writes, finish); called from open(). */
  static void install(long handle, Blob blob) {
    if (blob == null) {
      return;
    }
    CoocNative.restoreBegin(handle, blob.bytes);
    long offset = 0;
    for (byte[] range : blob.ranges) {
      CoocNative.restoreWrite(handle, offset, range.length, range);
      offset += range.length;
    }
    CoocNative.restoreFinish(handle, new long[10]);
    blob.ranges.clear();
  }
}
