// vs_aggregate_clips: the frame aggregation of videoseal.py:411-426 for every clip of a list in one launch (extract_messages).
// One workgroup per clip, thread t owns bits t, t + 256, ...; the rows of the clip are walked in order.  The row norms of the two *norm modes are
// block sums: per thread over its bits in order, then a halving tree over the 256 threads -- a function of nbits alone.  Everything is
// accumulated in fp64 (a few hundred values per clip: the rate does not matter) and rounded once, so the result is the correctly rounded
// aggregate up to one fp32 rounding whatever the dynamic range of the rows, and the same for any n and any launch shape.
#include "vs_common.h"

namespace {

constexpr int AGG_THREADS = 256, AGG_PER_THREAD = 4;      // nbits <= 1024

__global__ __launch_bounds__(AGG_THREADS) void aggregate_clips_kernel(const float* __restrict__ logits, const int64_t ld,
                                                                      const int32_t* __restrict__ first_row, const int nbits, const int mode,
                                                                      float* __restrict__ out) {
  __shared__ double red[AGG_THREADS];
  const int clip = blockIdx.x, tid = threadIdx.x;
  const int r0 = first_row[clip], r1 = first_row[clip + 1];      // block-uniform: the barriers below are reached by every thread
  double acc[AGG_PER_THREAD];
#pragma unroll
  for (int j = 0; j < AGG_PER_THREAD; ++j) acc[j] = 0.0;
  for (int r = r0; r < r1; ++r) {
    const float* row = logits + (int64_t)r * ld + 1;             // column 0 is the detection logit
    double x[AGG_PER_THREAD];
    double part = 0.0;
#pragma unroll
    for (int j = 0; j < AGG_PER_THREAD; ++j) {
      const int b = tid + j * AGG_THREADS;
      x[j] = b < nbits ? (double)row[b] : 0.0;
      part += mode == VS_AGG_L1NORM ? fabs(x[j]) : x[j] * x[j];
    }
    double w = 1.0;
    if (mode == VS_AGG_L1NORM || mode == VS_AGG_L2NORM) {
      red[tid] = part;
      __syncthreads();
      for (int s = AGG_THREADS / 2; s >= 1; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
      }
      w = mode == VS_AGG_L2NORM ? sqrt(red[0]) : red[0];
      __syncthreads();                                           // red is written again for the next row
    }
#pragma unroll
    for (int j = 0; j < AGG_PER_THREAD; ++j) acc[j] += mode == VS_AGG_SQUARED ? x[j] * fabs(x[j]) : x[j] * w;
  }
  const int rows = r1 - r0;
#pragma unroll
  for (int j = 0; j < AGG_PER_THREAD; ++j) {
    const int b = tid + j * AGG_THREADS;
    if (b < nbits) out[(int64_t)clip * nbits + b] = rows > 0 ? (float)(acc[j] / (double)rows) : 0.f;
  }
}

}  // namespace

extern "C" int vs_aggregate_clips(const float* logits, int64_t ld, const int32_t* first_row, int n, int nbits, int mode, float* out,
                                  void* stream) {
  VS_REQUIRE(logits && first_row && out && n > 0 && nbits > 0 && ld >= (int64_t)nbits + 1);
  VS_REQUIRE(mode >= VS_AGG_AVG && mode <= VS_AGG_L2NORM);
  if (nbits > AGG_THREADS * AGG_PER_THREAD) return VS_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(aggregate_clips_kernel, dim3((unsigned)n), dim3(AGG_THREADS), 0, (hipStream_t)stream, logits, ld, first_row, nbits, mode, out);
  return vs_launch_status();
}
