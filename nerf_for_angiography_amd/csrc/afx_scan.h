// afx_scan.h — the one workgroup-wide integer scan of the two-level compactions (device code only).
// Workgroups own chunks of consecutive elements and leave one partial each; ONE workgroup then scans the nb partials: thread t sums a run
// of ceil(nb / BLOCK) of them (scan_run), the BLOCK run sums are scanned (block_exclusive_scan) and the thread walks its run again from its
// prefix.  One level down the same scan, at BLOCK = 256, turns per-thread counts into positions inside a chunk.  Integers only: every
// correct scan gives the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace afx {

// The run of partials of thread threadIdx.x of a BLOCK-thread scanning workgroup: [b0, b1) of nb, empty (b0 == b1 == nb) behind the last one.
template <int BLOCK, class I>
__device__ __forceinline__ void scan_run(I nb, I& b0, I& b1) {
  const I per = (nb + (I)(BLOCK - 1)) / (I)BLOCK, lo = (I)threadIdx.x * per;
  b0 = lo < nb ? lo : nb;
  b1 = b0 + per < nb ? b0 + per : nb;
}

// x[q] becomes the sum of x[q] over the lower-numbered threads of the workgroup and total[q], in every thread, the sum over all of them,
// for N independent quantities at once (a quantity costs registers, not barriers).  An inclusive __shfl_up scan inside each 64-lane wave;
// the BLOCK / 64 wave totals go through LDS, where the first wave scans them: three barriers, the first of them before the LDS is
// written, so that a second call may follow at once.  (Every wave scanning the totals for itself saves a barrier and was measured slower
// in k_ray_offsets, 1024 threads and two 64-bit sums: the shuffles of 16 waves share one LDS pipe.  profiles/r25_scan_helper.md)
// EVERY thread of a one-dimensional workgroup of exactly BLOCK threads must call it.
template <int BLOCK, class T, int N>
__device__ __forceinline__ void block_exclusive_scan(T (&x)[N], T (&total)[N]) {
  constexpr int WAVES = BLOCK / 64;
  static_assert(BLOCK % 64 == 0 && WAVES >= 1 && WAVES <= 64, "whole waves, and one wave can scan their totals");
  __shared__ T wtot[N][WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T inc[N];
#pragma unroll
  for (int q = 0; q < N; ++q) {
    inc[q] = x[q];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const T v = __shfl_up(inc[q], d);
      if (lane >= d) inc[q] += v;
    }
  }
  __syncthreads();                                    // an earlier call's reads of wtot are over
  if (lane == 63) {
#pragma unroll
    for (int q = 0; q < N; ++q) wtot[q][wave] = inc[q];
  }
  __syncthreads();
  if (wave == 0) {                                    // wtot becomes its own inclusive scan
#pragma unroll
    for (int q = 0; q < N; ++q) {
      T a = lane < WAVES ? wtot[q][lane] : (T)0;
#pragma unroll
      for (int d = 1; d < WAVES; d <<= 1) {
        const T v = __shfl_up(a, d);
        if (lane >= d) a += v;
      }
      if (lane < WAVES) wtot[q][lane] = a;
    }
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < N; ++q) {
    x[q] = (wave ? wtot[q][wave - 1] : (T)0) + inc[q] - x[q];
    total[q] = wtot[q][WAVES - 1];
  }
}

}  // namespace afx
