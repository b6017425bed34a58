// cooc_window.h — the tumbling-window assignment, one expression for the host operator (cooc_stream.cpp) and the
// device log preparation (cooc_ingest_dev.hip), so that the two cannot drift.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace cooc {

// Flink TumblingEventTimeWindows.assignWindows with offset 0 [3P, Flink 1.3.2]:
// start = ts - (ts - offset + size) % size (Java remainder), maxTimestamp = start + size - 1.
// No overflow for ts in [Long.MIN_VALUE + 2 * size, Long.MAX_VALUE - 2 * size].
__host__ __device__ inline int64_t window_max_ts(int64_t ts, int64_t size) {
  const int64_t start = ts - (ts + size) % size;
  return start + size - 1;
}

}  // namespace cooc
