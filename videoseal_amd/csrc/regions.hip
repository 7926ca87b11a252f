// Region-wise decoding (include/videoseal_regions.h): what the label map of vs_embed_tail_regions needs on the way back.
//   vs_pixel_vote_regions : votes, pixel counts and logit sums of all R regions in ONE pass over the maps of a pixel-wise extractor
//   vs_label_boxes        : bounding boxes of the labels, for per-frame extractors that look at a crop per region
// The region-wise tail itself is a mode of the tile body in shell.hip.
#include "vs_common.h"
#include "videoseal_regions.h"
#include <climits>

namespace {

// ---- pixel vote.  Workgroup = (group of VKG channels, chunk of VCHUNK map pixels, frame).  A thread walks the chunk 256 pixels apart: it finds
// the pixel's label once (two integer divisions when the label map has another size than the maps), reads the VKG logits of the pixel -- every
// element of preds is read by exactly one thread of one workgroup, whatever R is -- and adds them into the registers of that label: R x VKG
// float64 sums and int counts, selected by compare (no indexed register file, no scratch).  The workgroup's totals go to `partial` in a fixed
// order (lanes by shuffles, then the four waves); vote_regions_finish_kernel adds the chunks in ascending order.  No atomics anywhere.
constexpr int VKG = 4, VCHUNK = 8192, VR = VS_REGIONS_MAX;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// partial: [B][NC][R][2 K + 1] doubles: (sum, votes) per channel, then the region's pixel count
__global__ __launch_bounds__(256) void vote_regions_kernel(const float* __restrict__ preds, const int64_t bstride, const unsigned char* __restrict__ labels,
                                                           const int K, const int Sh, const int Sw, const int H, const int W, const int R,
                                                           const float threshold, double* __restrict__ partial) {
  __shared__ double red_s[4][VR][VKG];
  __shared__ int red_v[4][VR][VKG + 1];
  const int kg = blockIdx.x, ch = blockIdx.y, b = blockIdx.z, NC = gridDim.y;
  const int HW = Sh * Sw;
  const int p0 = ch * VCHUNK, p1 = min(HW, p0 + VCHUNK);
  const float* pr = preds + (int64_t)b * bstride + (int64_t)kg * VKG * HW;
  const unsigned char* lab = labels + (int64_t)b * H * W;
  const bool same = H == Sh && W == Sw;
  const int nk = min(VKG, K - kg * VKG);              // channels of this group (the last group may be short)
  double s[VR][VKG];
  int v[VR][VKG], n[VR];
#pragma unroll
  for (int r = 0; r < VR; ++r) {
    n[r] = 0;
#pragma unroll
    for (int j = 0; j < VKG; ++j) { s[r][j] = 0.0; v[r][j] = 0; }
  }
  for (int p = p0 + (int)threadIdx.x; p < p1; p += 256) {
    int li = p;
    if (!same) {
      const unsigned y = (unsigned)p / (unsigned)Sw, x = (unsigned)p - y * (unsigned)Sw;
      const unsigned ly = ((2u * y + 1u) * (unsigned)H) / (2u * (unsigned)Sh), lx = ((2u * x + 1u) * (unsigned)W) / (2u * (unsigned)Sw);
      li = (int)(ly * (unsigned)W + lx);            // ly < H and lx < W: (2 y + 1) H < 2 Sh H
    }
    const unsigned l = lab[li];
    float val[VKG];
#pragma unroll
    for (int j = 0; j < VKG; ++j) val[j] = j < nk ? pr[(int64_t)j * HW + p] : 0.f;       // guarded: nothing past channel K - 1 is read
    if (l == 0u || l > (unsigned)R) continue;
#pragma unroll
    for (int r = 0; r < VR; ++r) {
      const bool hit = l == (unsigned)(r + 1);
      n[r] += hit;
#pragma unroll
      for (int j = 0; j < VKG; ++j) {
        s[r][j] += hit ? (double)val[j] : 0.0;
        v[r][j] += hit && val[j] > threshold;
      }
    }
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int r = 0; r < VR; ++r)
    if (r < R) {
#pragma unroll
      for (int j = 0; j < VKG; ++j) {
        const double ts = wave_sum(s[r][j]);
        const int tv = wave_sum(v[r][j]);
        if (lane == 0) { red_s[wave][r][j] = ts; red_v[wave][r][j] = tv; }
      }
      const int tn = wave_sum(n[r]);
      if (lane == 0) red_v[wave][r][VKG] = tn;
    }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < VR * (VKG + 1)) {
    const int r = t / (VKG + 1), j = t - r * (VKG + 1);
    if (r < R) {
      double* out = partial + (((int64_t)b * NC + ch) * R + r) * (2 * K + 1);
      if (j < VKG) {
        if (j < nk) {
          const int k = kg * VKG + j;
          out[2 * k] = ((red_s[0][r][j] + red_s[1][r][j]) + red_s[2][r][j]) + red_s[3][r][j];
          out[2 * k + 1] = (double)(red_v[0][r][j] + red_v[1][r][j] + red_v[2][r][j] + red_v[3][r][j]);
        }
      } else if (kg == 0) {
        out[2 * K] = (double)(red_v[0][r][VKG] + red_v[1][r][VKG] + red_v[2][r][VKG] + red_v[3][r][VKG]);
      }
    }
  }
}

// workgroup = (frame, region); a thread adds the chunks of its channels in ascending order (counts are whole numbers below 2^31: exact in float64)
__global__ __launch_bounds__(256) void vote_regions_finish_kernel(const double* __restrict__ partial, const int NC, const int K, const int R,
                                                                  int* __restrict__ votes, int* __restrict__ nsel, double* __restrict__ sums) {
  const int r = blockIdx.x, b = blockIdx.y;
  const int64_t row = 2 * (int64_t)K + 1;
  const double* p = partial + ((int64_t)b * NC * R + r) * row;
  for (int k = threadIdx.x; k <= K; k += 256) {
    if (k == K) {
      double c = 0.0;
      for (int i = 0; i < NC; ++i) c += p[(int64_t)i * R * row + 2 * K];
      nsel[(int64_t)b * R + r] = (int)c;
    } else {
      double sm = 0.0, vt = 0.0;
      for (int i = 0; i < NC; ++i) {
        sm += p[(int64_t)i * R * row + 2 * k];
        vt += p[(int64_t)i * R * row + 2 * k + 1];
      }
      sums[((int64_t)b * R + r) * K + k] = sm;
      votes[((int64_t)b * R + r) * K + k] = (int)vt;
    }
  }
}

// ---- label boxes.  Workgroup = a band of rows of one frame.  A thread keeps the box of every label in registers (selected by compare), the
// workgroup merges them in LDS and sends one integer min / max per present label and side to the frame's boxes.
constexpr int BOX_ROWS = 32;

__global__ __launch_bounds__(256) void label_boxes_init_kernel(int* __restrict__ boxes, const int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) boxes[i] = (i & 3) < 2 ? INT_MAX : 0;
}

__global__ __launch_bounds__(256) void label_boxes_kernel(const unsigned char* __restrict__ labels, const int H, const int W, const int R,
                                                          int* __restrict__ boxes) {
  __shared__ int sb[VR][4];
  const int f = blockIdx.y, ya = blockIdx.x * BOX_ROWS, yb = min(H, ya + BOX_ROWS);
  if (threadIdx.x < VR * 4) sb[threadIdx.x >> 2][threadIdx.x & 3] = (threadIdx.x & 3) < 2 ? INT_MAX : 0;
  __syncthreads();
  const unsigned char* lab = labels + (int64_t)f * H * W;
  int y0[VR], x0[VR], y1[VR], x1[VR];
#pragma unroll
  for (int r = 0; r < VR; ++r) { y0[r] = INT_MAX; x0[r] = INT_MAX; y1[r] = 0; x1[r] = 0; }
  const int64_t ia = (int64_t)ya * W, ib = (int64_t)yb * W;
  for (int64_t i = ia + threadIdx.x; i < ib; i += 256) {
    const unsigned l = lab[i];
    if (l == 0u || l > (unsigned)R) continue;
    const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
#pragma unroll
    for (int r = 0; r < VR; ++r)
      if (l == (unsigned)(r + 1)) {
        y0[r] = min(y0[r], y); x0[r] = min(x0[r], x); y1[r] = max(y1[r], y + 1); x1[r] = max(x1[r], x + 1);
      }
  }
#pragma unroll
  for (int r = 0; r < VR; ++r)
    if (y1[r] > 0) {
      atomicMin(&sb[r][0], y0[r]); atomicMin(&sb[r][1], x0[r]); atomicMax(&sb[r][2], y1[r]); atomicMax(&sb[r][3], x1[r]);
    }
  __syncthreads();
  if (threadIdx.x < VR * 4) {
    const int r = threadIdx.x >> 2, j = threadIdx.x & 3;
    if (r < R && sb[r][2] > 0) {
      int* dst = boxes + ((int64_t)f * R + r) * 4 + j;
      if (j < 2) atomicMin(dst, sb[r][j]);
      else atomicMax(dst, sb[r][j]);
    }
  }
}

// a label without a pixel: (INT_MAX, INT_MAX, 0, 0) -> (0, 0, 0, 0)
__global__ __launch_bounds__(256) void label_boxes_finish_kernel(int* __restrict__ boxes, const int n_boxes) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n_boxes && boxes[4 * i + 2] == 0) { boxes[4 * i] = 0; boxes[4 * i + 1] = 0; boxes[4 * i + 3] = 0; }
}

}  // namespace

extern "C" int64_t vs_pixel_vote_regions_partial_doubles(int B, int K, int64_t HW, int R) {
  if (B <= 0 || K <= 0 || HW <= 0 || R < 1 || R > VS_REGIONS_MAX) return -1;
  return (int64_t)B * cdiv64(HW, VCHUNK) * R * (2 * (int64_t)K + 1);
}

extern "C" int vs_pixel_vote_regions(const float* preds, int64_t batch_stride, const uint8_t* labels, int B, int K, int S_h, int S_w, int H, int W,
                                     int R, float threshold, int32_t* votes, int32_t* nsel, double* sums, double* partial, void* stream) {
  VS_REQUIRE(preds && labels && votes && nsel && sums && partial);
  VS_REQUIRE(B > 0 && K > 0 && S_h > 0 && S_w > 0 && H > 0 && W > 0 && R >= 1 && R <= VS_REGIONS_MAX);
  VS_REQUIRE((int64_t)S_h * S_w <= INT_MAX && (int64_t)H * W <= INT_MAX);
  VS_REQUIRE(2 * (int64_t)S_h * H <= INT_MAX && 2 * (int64_t)S_w * W <= INT_MAX);       // (2 y + 1) H in 32-bit arithmetic
  const int NC = (int)cdiv64((int64_t)S_h * S_w, VCHUNK);
  VS_REQUIRE(NC <= 65535 && B <= 65535);
  hipLaunchKernelGGL(vote_regions_kernel, dim3((K + VKG - 1) / VKG, NC, B), dim3(256), 0, (hipStream_t)stream, preds, batch_stride, labels, K, S_h,
                     S_w, H, W, R, threshold, partial);
  if (const int rc = vs_launch_status(); rc != VS_OK) return rc;
  hipLaunchKernelGGL(vote_regions_finish_kernel, dim3(R, B), dim3(256), 0, (hipStream_t)stream, partial, NC, K, R, votes, nsel, sums);
  return vs_launch_status();
}

extern "C" int vs_label_boxes(const uint8_t* labels, int F, int H, int W, int R, int32_t* boxes, void* stream) {
  VS_REQUIRE(labels && boxes && F > 0 && H > 0 && W > 0 && R >= 1 && R <= VS_REGIONS_MAX && F <= 65535);
  const int n = F * R * 4;
  hipLaunchKernelGGL(label_boxes_init_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, boxes, n);
  hipLaunchKernelGGL(label_boxes_kernel, dim3((H + BOX_ROWS - 1) / BOX_ROWS, F), dim3(256), 0, (hipStream_t)stream, labels, H, W, R, boxes);
  hipLaunchKernelGGL(label_boxes_finish_kernel, dim3((F * R + 255) / 256), dim3(256), 0, (hipStream_t)stream, boxes, F * R);
  return vs_launch_status();
}
