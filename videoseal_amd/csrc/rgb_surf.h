// Packed RGB frames as capture and image code hold them: vs_resize_pre and vs_embed_tail (shell.hip) on pixels of 3, 4, 6 or 8 bytes and on the
// 10:10:10:2 word, alpha / X carried through bit for bit.  Four kernels (resize and tail, each as a tile form and a row-streaming form), one
// body per kernel, a surface trait per LAYOUT; rgbpack.hip instantiates the five layouts and holds the entry points.
//   layout          formats                          stored word       depth
//   RgbSurf<3, 0>   rgb24, bgr24                     3 x uint8         8
//   RgbSurf<4, 0>   rgba, bgra, argb, abgr           4 x uint8         8
//   RgbSurf<6, 0>   rgb48, bgr48                     3 x uint16 (LE)   16
//   RgbSurf<8, 0>   rgba64, bgra64                   4 x uint16 (LE)   16
//   RgbSurf<4, 1>   x2rgb10, x2bgr10                 one uint32 (LE)   10
// Where R, G and B sit inside the pixel (component index, or bit shift inside the 10:10:10:2 word) is a kernel ARGUMENT (RgbPos): twelve
// formats, five instantiations of every kernel.  A pixel travels as `Raw`: its little-endian bytes 0 - 3 in w0, 4 - 7 in w1.
// Decode: component = float(code) / float(top), top = 2^depth - 1, correctly rounded (u8_unit's Newton step of shell.hip, which is exact for
// 255, 1023 and 65535: tests/test_rgbpack_cpu.py and test_gpu_rgbpack.py check every code).  Encode: floor(clamp(v, 0, 1) * top) -- the
// truncation of Px<unsigned char>::st.  floor((c / top) * top) == c for every code of the three depths, so a pixel the watermark leaves alone
// keeps its word.  The bits of a pixel that are not R, G or B (alpha, X) are copied from the source pixel and never enter arithmetic.
// Frame bytes move as 16-byte PIECES at byte offsets 16 k of a row: one 16-byte access where the piece lies inside the row's W x BPP bytes and
// its address is aligned, byte by byte, guarded, elsewhere -- any base address and any byte pitch work (a 16-bit word may sit at an odd
// address), bytes between a row's end and its pitch are neither used nor written.  A 3- or 6-byte pixel straddles pieces: the tail kernels
// stage a row's pieces in LDS as bytes and read pixels from there; a resize load task is 16 pixels = BPP whole pieces held in registers.
// Between decode and encode the filter taps, the JND, the key-frame expansion and the blend are the expressions of the fp32 kernels of the
// same form in the same order (shell_common.h): a packed clip gives the bits of the fp32 path on its decoded frames.
#pragma once
#include "tail_phases.h"

namespace {

struct RgbPlane { const unsigned char* p; int64_t pitch, fs; };       // bytes
struct RgbPos { int r, g, b; };                                       // component index of R, G, B inside the pixel (10:10:10:2: bit shift)
struct RgbGeo { RgbPlane s, d; RgbPos pos; };
struct Raw { unsigned w0, w1; };                                      // a pixel's bytes 0 - 3 and 4 - 7, little-endian

template <int BPP_, bool X2_>
struct RgbSurf {
  static_assert((BPP_ == 3 || BPP_ == 4 || BPP_ == 6 || BPP_ == 8) && (!X2_ || BPP_ == 4), "3, 4, 6 or 8 bytes per pixel, or the 10:10:10:2 word");
  static constexpr int BPP = BPP_;
  static constexpr bool X2 = X2_;
  static constexpr int DEPTH = X2_ ? 10 : (BPP_ >= 6 ? 16 : 8);
  static constexpr unsigned TOPU = (1u << DEPTH) - 1u;
  static constexpr int ROWB = TTW * BPP_ + 32;              // bytes of a tail window row: one piece, the tile's 256 pixels, one piece (2 BPP <= 16: the halo fits)
  static constexpr int NPR = ROWB / 16;                     // its pieces
  static constexpr int PPR = TTW * BPP_ / 16;               // pieces of an output row of 256 pixels

  // float(code) / float(top), correctly rounded: one Newton correction of code * (1 / top)
  static __device__ __forceinline__ float unit(const float u) {
    constexpr float top = (float)TOPU;
    const float r = 1.0f / top;
    const float q = u * r;
    const float rem = __builtin_fmaf(-q, top, u);
    return __builtin_fmaf(rem, r, q);
  }
  // (values, not references, and both words computed before the choice: a choice between two members' ADDRESSES would park the pixel in scratch)
  static __device__ __forceinline__ unsigned code(const unsigned w0, const unsigned w1, const int pos) {
    if (X2_) return (w0 >> pos) & 0x3ffu;
    if (DEPTH == 8) return (w0 >> (8 * pos)) & 0xffu;
    const unsigned w = (pos & 2) ? w1 : w0;
    return (w >> (16 * (pos & 1))) & 0xffffu;
  }
  static __device__ __forceinline__ void decode(const Raw x, const RgbPos& pos, float (&rgb)[3]) {
    const unsigned w0 = x.w0, w1 = x.w1;
    rgb[0] = unit((float)code(w0, w1, pos.r));
    rgb[1] = unit((float)code(w0, w1, pos.g));
    rgb[2] = unit((float)code(w0, w1, pos.b));
  }
  static __device__ __forceinline__ void put(unsigned& w0, unsigned& w1, const int pos, const unsigned c) {
    if (X2_) { w0 = (w0 & ~(0x3ffu << pos)) | (c << pos); return; }
    if (DEPTH == 8) { w0 = (w0 & ~(0xffu << (8 * pos))) | (c << (8 * pos)); return; }
    const int sh = 16 * (pos & 1);
    const unsigned keep = ~(0xffffu << sh), n0 = (w0 & keep) | (c << sh), n1 = (w1 & keep) | (c << sh);
    const bool hi = (pos & 2) != 0;
    w0 = hi ? w0 : n0;
    w1 = hi ? n1 : w1;
  }
  // the source pixel with R, G, B replaced by floor(v * top), v already clamped to [0, 1]; every other bit is the source's
  static __device__ __forceinline__ Raw encode(const Raw x, const RgbPos& pos, const float (&v)[3]) {
    constexpr float top = (float)TOPU;
    unsigned w0 = x.w0, w1 = x.w1;
    put(w0, w1, pos.r, (unsigned)(v[0] * top));
    put(w0, w1, pos.g, (unsigned)(v[1] * top));
    put(w0, w1, pos.b, (unsigned)(v[2] * top));
    return Raw{w0, w1};
  }

  // 16 bytes from byte offset `off` of a row of `rowb` bytes; bytes outside the row read as zero
  static __device__ __forceinline__ uint4 ld16(const unsigned char* __restrict__ row, const int64_t off, const int64_t rowb) {
    const unsigned char* p = row + off;
    if (off >= 0 && off + 16 <= rowb && (reinterpret_cast<uintptr_t>(p) & 15) == 0) return *reinterpret_cast<const uint4*>(p);
    unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int q = 0; q < 16; ++q)
      if (off + q >= 0 && off + q < rowb) w[q >> 2] |= (unsigned)p[q] << (8 * (q & 3));
    return uint4{w[0], w[1], w[2], w[3]};
  }
  static __device__ __forceinline__ void st16(unsigned char* __restrict__ row, const int64_t off, const int64_t rowb, const unsigned char* __restrict__ lds) {
    unsigned char* p = row + off;
    if (off + 16 <= rowb && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
      *reinterpret_cast<uint4*>(p) = *reinterpret_cast<const uint4*>(lds);
      return;
    }
    const uint4 v = *reinterpret_cast<const uint4*>(lds);
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int q = 0; q < 16; ++q)
      if (off + q < rowb) p[q] = (unsigned char)(w[q >> 2] >> (8 * (q & 3)));
  }

  // pixel q (a compile-time constant after unrolling) of a task of 16 pixels held as BPP pieces
  static __device__ __forceinline__ unsigned dw(const uint4 (&v)[BPP_], const int i) {
    const uint4& u = v[(i >> 2) < BPP_ ? (i >> 2) : BPP_ - 1];
    const int e = i & 3;
    return e == 0 ? u.x : (e == 1 ? u.y : (e == 2 ? u.z : u.w));
  }
  static __device__ __forceinline__ Raw from_regs(const uint4 (&v)[BPP_], const int q) {
    if (BPP_ == 4) return Raw{dw(v, q), 0u};
    if (BPP_ == 8) return Raw{dw(v, 2 * q), dw(v, 2 * q + 1)};
    const int b0 = q * BPP_, j = b0 >> 2;                   // 3 or 6 bytes from byte b0: inside the dwords j, j + 1
    const unsigned lo = dw(v, j), hi = j + 1 < 4 * BPP_ ? dw(v, j + 1) : 0u;
    const unsigned long long t = (((unsigned long long)hi << 32) | lo) >> (8 * (b0 & 3));
    if (BPP_ == 3) return Raw{(unsigned)t & 0xffffffu, 0u};
    return Raw{(unsigned)t, (unsigned)(t >> 32) & 0xffffu};
  }
  // a pixel staged in LDS (p: its first byte; 4- and 8-byte pixels are aligned there, 6-byte ones to two bytes)
  static __device__ __forceinline__ Raw from_lds(const unsigned char* p) {
    if (BPP_ == 4) return Raw{*reinterpret_cast<const unsigned*>(p), 0u};
    if (BPP_ == 8) { const uint2 t = *reinterpret_cast<const uint2*>(p); return Raw{t.x, t.y}; }
    if (BPP_ == 6) {
      const unsigned short* h = reinterpret_cast<const unsigned short*>(p);
      return Raw{(unsigned)h[0] | ((unsigned)h[1] << 16), (unsigned)h[2]};
    }
    return Raw{(unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16), 0u};
  }
  static __device__ __forceinline__ void to_lds(unsigned char* p, const Raw& x) {
    if (BPP_ == 4) { *reinterpret_cast<unsigned*>(p) = x.w0; return; }
    if (BPP_ == 8) { *reinterpret_cast<uint2*>(p) = uint2{x.w0, x.w1}; return; }
    if (BPP_ == 6) {
      unsigned short* h = reinterpret_cast<unsigned short*>(p);
      h[0] = (unsigned short)(x.w0 & 0xffffu); h[1] = (unsigned short)(x.w0 >> 16); h[2] = (unsigned short)(x.w1 & 0xffffu);
      return;
    }
    p[0] = (unsigned char)(x.w0 & 0xffu); p[1] = (unsigned char)((x.w0 >> 8) & 0xffu); p[2] = (unsigned char)((x.w0 >> 16) & 0xffu);
  }
  // a pixel straight from the frame, byte by byte (the unstaged paths of the tile resize): any address
  static __device__ __forceinline__ Raw from_global(const unsigned char* __restrict__ p) {
    Raw x{0u, 0u};
#pragma unroll
    for (int i = 0; i < BPP_; ++i) {
      if (i < 4) x.w0 |= (unsigned)p[i] << (8 * i);
      else x.w1 |= (unsigned)p[i] << (8 * (i - 4));
    }
    return x;
  }
};

// Tile form of the resize: resize_pre_kernel (shell.hip) on packed pixels.  A workgroup owns 32 x 8 output pixels.  Staging: a task is 16
// pixels of one row (BPP whole pieces, from a column that is a multiple of 16: byte offset 16 BPP k), decoded from registers into the fp32
// window in LDS; the window of at most RS_WW x RS_WH pixels spans <= 9 tasks x 32 rows, taken in turn by the 256 threads.  A window that does
// not fit is filtered straight from the frame.  Taps, their order and the epilogue are resize_pre_tile's.
template <class SF>
__global__ __launch_bounds__(256) void resize_pre_rgb_kernel(RgbPlane s, RgbPos pos, int B, int H, int W, int oh, int ow, int antialias,
                                                             float* __restrict__ dst_rgb, float mul, float add, float* __restrict__ dst_key,
                                                             int key_step, int key_mode, float y0, float y1, float y2) {
  __shared__ float Lw[3 * RS_WH * RS_WW];
  constexpr int BPP = SF::BPP;
  const int ox0 = blockIdx.x * 32, oy0 = blockIdx.y * 8;
  const int b = blockIdx.z;
  const unsigned char* base = s.p + (int64_t)b * s.fs;
  const int64_t pitch = s.pitch, rowb = (int64_t)W * BPP;
  int x_lo, y_lo, x_hi, y_hi, n_;
  tap_range(ox0, W, ow, antialias, x_lo, n_);
  tap_range(min(ox0 + 31, ow - 1), W, ow, antialias, x_hi, n_);
  const int ww = x_hi + n_ - x_lo;
  tap_range(oy0, H, oh, antialias, y_lo, n_);
  tap_range(min(oy0 + 7, oh - 1), H, oh, antialias, y_hi, n_);
  const int wh = y_hi + n_ - y_lo;
  const bool staged = ww <= RS_WW && wh <= RS_WH;          // block-uniform
  if (staged) {
    const int pc0 = x_lo / 16, npc = ((x_lo + ww - 1) / 16) - pc0 + 1;
    for (int t = threadIdx.x; t < npc * wh; t += 256) {
      const int yy = t / npc, pi = t - yy * npc;
      const int col = (pc0 + pi) * 16;
      const unsigned char* rowp = base + (int64_t)(y_lo + yy) * pitch;          // (the window ends inside the frame)
      uint4 v[BPP];
#pragma unroll
      for (int i = 0; i < BPP; ++i) v[i] = SF::ld16(rowp, (int64_t)col * BPP + 16 * i, rowb);
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int xx = col + q - x_lo;
        if (xx >= 0 && xx < ww) {
          float rgb[3];
          SF::decode(SF::from_regs(v, q), pos, rgb);
#pragma unroll
          for (int c = 0; c < 3; ++c) Lw[(c * RS_WH + yy) * RS_WW + xx] = rgb[c];
        }
      }
    }
    __syncthreads();
  }
  const int ox = ox0 + (threadIdx.x & 31);
  const int oy = oy0 + (threadIdx.x >> 5);
  if (ox >= ow || oy >= oh) return;
  const Taps ty = make_taps(oy, H, oh, antialias), tx = make_taps(ox, W, ow, antialias);
  float acc[3] = {0.f, 0.f, 0.f};
  if (staged && tx.n <= MAXT) {
    float wxs[MAXT];
#pragma unroll
    for (int jx = 0; jx < MAXT; ++jx) wxs[jx] = jx < tx.n ? tap_w(tx, jx) : 0.f;
    const float* Lp = Lw + (ty.lo - y_lo) * RS_WW + (tx.lo - x_lo);
    for (int jy = 0; jy < ty.n; ++jy) {
      const float wy = tap_w(ty, jy);
      float r[3] = {0.f, 0.f, 0.f};
#pragma unroll
      for (int jx = 0; jx < MAXT; ++jx)
        if (jx < tx.n) {
#pragma unroll
          for (int c = 0; c < 3; ++c) r[c] = __builtin_fmaf(wxs[jx], Lp[(c * RS_WH + jy) * RS_WW + jx], r[c]);
        }
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] = __builtin_fmaf(wy, r[c], acc[c]);
    }
  } else if (tx.n > LONG_TAPS || ty.n > LONG_TAPS) {        // long filters: compensated sums, as resize_pre_kernel
    CompSum a3[3];
    for (int jy = 0; jy < ty.n; ++jy) {
      const float wy = tap_w(ty, jy);
      const unsigned char* rowp = base + (int64_t)(ty.lo + jy) * pitch;
      CompSum r3[3];
      for (int jx = 0; jx < tx.n; ++jx) {
        const float wx = tap_w(tx, jx);
        float rgb[3];
        SF::decode(SF::from_global(rowp + (int64_t)(tx.lo + jx) * BPP), pos, rgb);
#pragma unroll
        for (int c = 0; c < 3; ++c) r3[c].add(wx, rgb[c]);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) a3[c].add(wy, r3[c].value());
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] = a3[c].value();
  } else {
    for (int jy = 0; jy < ty.n; ++jy) {
      const float wy = tap_w(ty, jy);
      const unsigned char* rowp = base + (int64_t)(ty.lo + jy) * pitch;
      float r[3] = {0.f, 0.f, 0.f};
      for (int jx = 0; jx < tx.n; ++jx) {
        const float wx = tap_w(tx, jx);
        float rgb[3];
        SF::decode(SF::from_global(rowp + (int64_t)(tx.lo + jx) * BPP), pos, rgb);
#pragma unroll
        for (int c = 0; c < 3; ++c) r[c] = __builtin_fmaf(wx, rgb[c], r[c]);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] = __builtin_fmaf(wy, r[c], acc[c]);
    }
  }
  const int64_t opix = ((int64_t)oy * ow + ox);
  if (dst_rgb) {
    f32x4 v = {acc[0] * mul + add, acc[1] * mul + add, acc[2] * mul + add, 0.f};
    *reinterpret_cast<f32x4*>(dst_rgb + ((int64_t)b * oh * ow + opix) * 4) = v;
  }
  if (dst_key && (b % key_step) == 0) {
    f32x4 v;
    if (key_mode == 0) {
      const float y = y0 * acc[0] + y1 * acc[1] + y2 * acc[2];
      v = f32x4{y * 2.f - 1.f, 0.f, 0.f, 0.f};
    } else {
      v = f32x4{acc[0] * 2.f - 1.f, acc[1] * 2.f - 1.f, acc[2] * 2.f - 1.f, 0.f};
    }
    *reinterpret_cast<f32x4*>(dst_key + ((int64_t)(b / key_step) * oh * ow + opix) * 4) = v;
  }
}

// Row-streaming form of the resize: the structure of vs_rs::resize_stream_tile (resize_stream.h) with its own loader.  A workgroup owns OW
// output columns x a strip of output rows and walks the input rows eight at a time.  The window starts on a multiple of 16 columns (a byte
// offset that is a multiple of 16 for every BPP); a load task is 16 pixels of one of the group's eight rows = BPP pieces, requested one group
// ahead: <= 28 tasks x 8 rows, one per thread.  The thread that holds a task decodes its pixels straight from registers into the [8][3][INW]
// fp32 window.  This kernel keeps its OWN copy of the two passes (the note at the top of resize_stream.h says why): a change to the passes of
// resize_stream_tile belongs here as well.
constexpr int RGB_RS_ALIGN = 16;                           // window start and load task, in columns: the margin of vs_rs::rs_pick
template <class SF, int OW>
__global__ __launch_bounds__(256) void resize_pre_rgb_stream_kernel(RgbPlane s, RgbPos pos, int H, int W, int oh, int ow, int antialias,
                                                                    ResizePreEpi epi, int strip) {
  using namespace vs_rs;
  extern __shared__ __attribute__((aligned(16))) float rs_smem[];
  constexpr int INW = RsGeo<OW>::INW, MT = RsGeo<OW>::MT, RING = RsGeo<OW>::RING, NPART = 256 / OW, RPP = RS_GI / NPART;
  constexpr int BPP = SF::BPP, CW = 16;
  static_assert(INW % CW == 0 && RS_GI * (INW / CW) <= 256, "a task ends inside the window row; one load task per thread");
  float* In = rs_smem;                                   // [RS_GI][3][INW]
  float* Hr = rs_smem + RS_GI * 3 * INW;                 // [RING][3][OW]
  float* Wy = Hr + RING * 3 * OW;                        // [RS_WTAB_ROWS][MT] vertical weights | first row | tap count
  int* WyLo = reinterpret_cast<int*>(Wy + RS_WTAB_ROWS * MT);
  int* WyN = WyLo + RS_WTAB_ROWS;
  const int ox0 = blockIdx.x * OW, oy0 = blockIdx.y * strip, b = blockIdx.z;
  const int oy_end = min(oh, oy0 + strip);
  const unsigned char* base = s.p + (int64_t)b * s.fs;
  const int64_t pitch = s.pitch, rowb = (int64_t)W * BPP;
  const int tid = threadIdx.x;
  const int oxl = tid & (OW - 1), part = tid / OW;
  const int ox = min(ox0 + oxl, ow - 1);
  const bool ox_ok = ox0 + oxl < ow;
  const bool wtab = strip <= RS_WTAB_ROWS;               // block-uniform
  if (wtab && tid < oy_end - oy0) {
    const Taps t = make_taps(oy0 + tid, H, oh, antialias);
    WyLo[tid] = t.lo;
    WyN[tid] = t.n;
    for (int q = 0; q < MT; ++q) Wy[tid * MT + q] = q < t.n ? tap_w(t, q) : 0.f;
  }
  int x_lo, x_hi, n_;
  tap_range(ox0, W, ow, antialias, x_lo, n_);
  tap_range(min(ox0 + OW - 1, ow - 1), W, ow, antialias, x_hi, n_);
  const int xa = x_lo & ~(CW - 1);                       // LDS column 0 <-> frame column xa
  const int ww = min(x_hi + n_ - xa, INW);               // (<= INW: rs_pick with a margin of 16)
  const int npc = (ww + CW - 1) / CW;
  int y_lo, y_hi;
  tap_range(oy0, H, oh, antialias, y_lo, n_);
  tap_range(oy_end - 1, H, oh, antialias, y_hi, n_);
  const int y_end = y_hi + n_;
  const Taps tx = make_taps(ox, W, ow, antialias);
  float wxs[MT];
#pragma unroll
  for (int jx = 0; jx < MT; ++jx) wxs[jx] = jx < tx.n ? tap_w(tx, jx) : 0.f;
  const int xoff = tx.lo - xa;

  const bool loader = tid < RS_GI * npc;
  const int ri = tid / npc, pi = tid - ri * npc;          // row of the group, task
  uint4 pv[BPP];
  auto load_group = [&](const int r0) __attribute__((always_inline)) {
    const int row = r0 + ri;
#pragma unroll
    for (int i = 0; i < BPP; ++i) pv[i] = uint4{0u, 0u, 0u, 0u};
    if (loader && row < y_end && row < H) {
      const unsigned char* rowp = base + (int64_t)row * pitch;
#pragma unroll
      for (int i = 0; i < BPP; ++i) pv[i] = SF::ld16(rowp, (int64_t)(xa + CW * pi) * BPP + 16 * i, rowb);
    }
  };
  int oy_next = oy0 + part;
  load_group(y_lo);
  for (int r0 = y_lo; r0 < y_end; r0 += RS_GI) {
    if (loader) {       // whole tasks, four pixels per LDS store (columns past ww and rows past y_end receive values nobody reads)
#pragma unroll
      for (int k4 = 0; k4 < CW / 4; ++k4) {
        float px[3][4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float rgb[3];
          SF::decode(SF::from_regs(pv, 4 * k4 + e), pos, rgb);
#pragma unroll
          for (int c = 0; c < 3; ++c) px[c][e] = rgb[c];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c)
          *reinterpret_cast<f32x4*>(In + (ri * 3 + c) * INW + CW * pi + 4 * k4) = f32x4{px[c][0], px[c][1], px[c][2], px[c][3]};
      }
    }
    if (r0 + RS_GI < y_end) load_group(r0 + RS_GI);       // in flight during the two passes below
    __syncthreads();
#pragma unroll
    for (int q = 0; q < RPP; ++q) {
      const int rl = part * RPP + q;
      const int row = r0 + rl;
      if (row < y_end) {
        float r[3] = {0.f, 0.f, 0.f};
        const float* Lp = In + rl * 3 * INW + xoff;
#pragma unroll
        for (int jx = 0; jx < MT; ++jx)
          if (jx < tx.n) {
#pragma unroll
            for (int c = 0; c < 3; ++c) r[c] = __builtin_fmaf(wxs[jx], Lp[c * INW + jx], r[c]);
          }
#pragma unroll
        for (int c = 0; c < 3; ++c) Hr[((row & (RING - 1)) * 3 + c) * OW + oxl] = r[c];
      }
    }
    __syncthreads();
    const int done = min(r0 + RS_GI, y_end);
    while (oy_next < oy_end) {
      float acc[3] = {0.f, 0.f, 0.f};
      if (wtab) {
        const int tl = WyLo[oy_next - oy0], tn = WyN[oy_next - oy0];
        if (tl + tn > done) break;
        const float* wyp = Wy + (oy_next - oy0) * MT;
        for (int jy = 0; jy < tn; ++jy) {
          const float wy = wyp[jy];
          const float* hp = Hr + (((tl + jy) & (RING - 1)) * 3) * OW + oxl;
#pragma unroll
          for (int c = 0; c < 3; ++c) acc[c] = __builtin_fmaf(wy, hp[c * OW], acc[c]);
        }
      } else {
        const Taps ty = make_taps(oy_next, H, oh, antialias);
        if (ty.lo + ty.n > done) break;
        for (int jy = 0; jy < ty.n; ++jy) {
          const float wy = tap_w(ty, jy);
          const float* hp = Hr + (((ty.lo + jy) & (RING - 1)) * 3) * OW + oxl;
#pragma unroll
          for (int c = 0; c < 3; ++c) acc[c] = __builtin_fmaf(wy, hp[c * OW], acc[c]);
        }
      }
      if (ox_ok) epi(b, oy_next, ox, acc);
      oy_next += NPART;
    }
  }
}

// Tile form of the tail: embed_tail_kernel (shell.hip, its 43-tap form) on packed pixels.  Workgroup = 256 columns x 16 rows of one frame.  The
// tile's bytes + a 2-pixel halo (20 rows of ROWB bytes from byte x0 BPP - 16) are staged in LDS once, piece by piece; luminance and blend
// both read the pixel from there.  A thread owns one column; the watermarked pixel is written over the source pixel in LDS as its stored word
// (nobody else reads that pixel after the luminance phase; alpha / X are the word's other bits), and the tile's 16 rows leave as 16 BPP
// pieces each.  LDS: 20 x ROWB bytes (16 KB at 3 B/pixel, 41.6 KB at 8) + 20.8 KB luminance + 19.6 KB watermark window = 56.8 / 61.9 / 72.1 /
// 82.4 KB for 3 / 4 / 6 / 8 B/pixel: two workgroups per CU of 160 KB, one at 8 B/pixel -- this form serves frames too small for the
// row-streaming one and variant = 1.
constexpr int RGB_NVR = TTH + 2 * HALO;
template <class SF>
__global__ __launch_bounds__(256) void embed_tail_rgb_kernel(TailArgs a, JndTaps k, RgbGeo g) {
  constexpr int BPP = SF::BPP, ROWB = SF::ROWB, NPR = SF::NPR, PPR = SF::PPR, NVR = RGB_NVR;
  __shared__ __attribute__((aligned(16))) unsigned char WS[NVR * ROWB];
  __shared__ float L[TLW * NVR];
  __shared__ float Dw[3 * DW_W * DW_H];
  __shared__ int ty_lo[TTH], ty_n[TTH];
  __shared__ float ty_w[TTH][4];
  __shared__ int s_xhi, s_nmax, s_xlo;
  const int x0 = blockIdx.x * TTW, y0 = blockIdx.y * TTH, f = blockIdx.z;
  const bool full_jnd = a.attenuate && !a.hmap_lowres;
  const int64_t rowb = (int64_t)a.W * BPP;
  const unsigned char* sbase = g.s.p + (int64_t)f * g.s.fs;
  if (threadIdx.x == 0) { s_xhi = 0; s_nmax = 0; }
  {     // frame bytes -> LDS: NVR x NPR pieces in batches of four per thread, the loads of a batch issued before its stores
    constexpr int NTASK = NVR * NPR;
    for (int t0 = 0; t0 < NTASK; t0 += 4 * 256) {
      uint4 v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int t = t0 + threadIdx.x + 256 * i;
        v[i] = uint4{0u, 0u, 0u, 0u};
        if (t < NTASK) {
          const int r = t / NPR, p = t - r * NPR;
          const int gy = y0 - HALO + r;
          const bool need = full_jnd || (r >= HALO && r < HALO + TTH);
          if (need && gy >= 0 && gy < a.H) v[i] = SF::ld16(sbase + (int64_t)gy * g.s.pitch, (int64_t)x0 * BPP - 16 + 16 * p, rowb);
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int t = t0 + threadIdx.x + 256 * i;
        if (t < NTASK) *reinterpret_cast<uint4*>(WS + 16 * t) = v[i];
      }
    }
  }
  __syncthreads();
  // the stored pixel at tile row rr (0 .. NVR - 1 <-> frame row y0 - 2 + rr) and tile column tc (-2 .. 257 <-> frame column x0 + tc)
  auto at = [&](const int rr, const int tc) __attribute__((always_inline)) -> unsigned char* { return WS + rr * ROWB + 16 + tc * BPP; };
  if (full_jnd) {       // luminance of the tile + halo, zero outside the frame (conv zero padding)
    auto lum_column = [&](const int lxx) __attribute__((always_inline)) {
      const int gx = x0 + lxx - HALO;
#pragma unroll 4
      for (int rr = 0; rr < NVR; ++rr) {
        const int gy = y0 + rr - HALO;
        float v = 0.f;
        if (gx >= 0 && gx < a.W && gy >= 0 && gy < a.H) {
          float rgb[3];
          SF::decode(SF::from_lds(at(rr, lxx - HALO)), g.pos, rgb);
          v = lum255(rgb[0], rgb[1], rgb[2]);
        }
        L[rr * TLW + lxx] = v;
      }
    };
    lum_column(threadIdx.x + HALO);
    if (threadIdx.x < 2 * HALO) lum_column(threadIdx.x < HALO ? threadIdx.x : TTW + threadIdx.x);
  }
  const int lx = threadIdx.x;
  const int x = x0 + lx;
  const bool xin = x < a.W;
  const Taps tx = make_taps(xin ? x : a.W - 1, a.Sw, a.W, a.antialias);
  float wxs[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) wxs[j] = j < tx.n ? tap_w(tx, j) : 0.f;
  if (xin) { atomicMax(&s_xhi, tx.lo + tx.n); atomicMax(&s_nmax, tx.n); }
  if (threadIdx.x == 0) s_xlo = tx.lo;
  if (threadIdx.x < TTH) {
    const int yy = y0 + threadIdx.x;
    const Taps tp = make_taps(yy < a.H ? yy : a.H - 1, a.Sh, a.H, a.antialias);
    ty_lo[threadIdx.x] = tp.lo;
    ty_n[threadIdx.x] = tp.n;
#pragma unroll
    for (int j = 0; j < 4; ++j) ty_w[threadIdx.x][j] = j < tp.n ? tap_w(tp, j) : 0.f;
    if (yy < a.H) atomicMax(&s_nmax, tp.n);
  }
  __syncthreads();

  const KeyMix km = key_mix(a, f, a.Cd);                 // value = wa*key[ka] + wb*key[kb]
  const float wa = km.wa, wb = km.wb;
  const float *dka = km.dka, *dkb = km.dkb, *hml = km.hml;
  const int splane = a.Sh * a.Sw;

  const int lasty = min(TTH, a.H - y0) - 1;
  const int wx0 = s_xlo, wy0 = ty_lo[0];
  const int dww = s_xhi - wx0, dwh = ty_lo[lasty] + ty_n[lasty] - wy0;
  const int blk_n = s_nmax;
  const bool staged = blk_n <= 4 && dww <= DW_W && dwh <= DW_H;
  if (staged) {
    for (int i = threadIdx.x; i < dwh * dww; i += 256) {
      const int yy = i / dww, xx = i - yy * dww;
      const int sp = (wy0 + yy) * a.Sw + wx0 + xx;
      const float hm = hml ? hml[sp] : 1.f;
      for (int c = 0; c < a.Cd; ++c) {
        float v = wa * dka[c * splane + sp];
        if (wb != 0.f) v = __builtin_fmaf(wb, dkb[c * splane + sp], v);
        Dw[c * (DW_W * DW_H) + yy * DW_W + xx] = hm * v;
      }
    }
  }
  __syncthreads();      // L, Dw

  auto tap = [&](const int sp, const float wx, float (&r)[3]) __attribute__((always_inline)) {
    const float hm = hml ? hml[sp] : 1.f;
    for (int c = 0; c < a.Cd; ++c) {
      float v = wa * dka[c * splane + sp];
      if (wb != 0.f) v += wb * dkb[c * splane + sp];
      r[c] += wx * (hm * v);
    }
  };
  if (xin) {
    for (int ly = 0; ly <= lasty; ++ly) {
      const int y = y0 + ly;
      unsigned char* pp = at(ly + HALO, lx);
      const Raw src = SF::from_lds(pp);
      float px[3];
      SF::decode(src, g.pos, px);
      float d[3] = {0.f, 0.f, 0.f};
      const int ylo = ty_lo[ly], yn = ty_n[ly];
      if (staged) {
        const int basep = (ylo - wy0) * DW_W + (tx.lo - wx0);
        if (blk_n <= 3) tail_taps<3, DW_H>(d, Dw, a.Cd, basep, tx.n, yn, wxs, ty_w[ly]);
        else tail_taps<4, DW_H>(d, Dw, a.Cd, basep, tx.n, yn, wxs, ty_w[ly]);
      } else {
        const Taps ty = make_taps(y, a.Sh, a.H, a.antialias);
        for (int jy = 0; jy < ty.n; ++jy) {
          const float wy = tap_w(ty, jy);
          float r[3] = {0.f, 0.f, 0.f};
          for (int jx = 0; jx < tx.n; ++jx) tap((ty.lo + jy) * a.Sw + tx.lo + jx, tap_w(tx, jx), r);
          for (int c = 0; c < a.Cd; ++c) d[c] += wy * r[c];
        }
      }
      float hm = 1.f;
      if (full_jnd) {
        hm = jnd_at(L, TLW, lx + HALO, ly + HALO, k);
        for (int c = 0; c < a.Cd; ++c) d[c] = hm * d[c];
      }
      float v[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float t = blend_px(a.scaling_i, a.scaling_w, px[c], d[a.Cd == 1 ? 0 : c], hm, false);
        v[c] = t <= 0.f ? 0.f : (t >= 1.f ? 1.f : t);
      }
      SF::to_lds(pp, SF::encode(src, g.pos, v));
    }
  }
  __syncthreads();      // the tile's output words
  unsigned char* dbase = const_cast<unsigned char*>(g.d.p) + (int64_t)f * g.d.fs;
  for (int t = threadIdx.x; t < TTH * PPR; t += 256) {
    const int r = t / PPR, pc = t - r * PPR;
    const int64_t off = (int64_t)x0 * BPP + 16 * pc;
    if (y0 + r < a.H && off < rowb) SF::st16(dbase + (int64_t)(y0 + r) * g.d.pitch, off, rowb, WS + (r + HALO) * ROWB + 16 + 16 * pc);
  }
}

// Row-streaming form of the tail: embed_tail_stream_kernel's structure (shell.hip: 256 columns x a strip of rows walked in groups of SG = 4,
// luminance ring, accumulators of the separable JND stencils with the re-evaluation at the jump, double-buffered watermark window, ONE
// barrier per group) with the frame's bytes staged through LDS as 16-byte pieces, as embed_tail_yuv_stream_kernel does it.  A group's 4 rows
// are 4 NPR pieces (200 at 3 B/pixel: one per thread; 520 at 8: three), requested two groups ahead of their use: loaded during group it - 1,
// written to the byte stage before the barrier of group it, read by every thread (own column, halo columns) at the top of group it + 1.  The
// pixel's stored word waits in registers beside its decoded value until its output row is complete two rows later, so that alpha / X reach
// the output word without passing through floats.  The group's output words (4 x 256 pixels) are collected in LDS and leave after the next
// barrier as 4 x 16 BPP pieces (<= two per thread).  Static LDS: 2 x 4 x ROWB + 2 x 4 x 256 BPP bytes = 13.3 KB (3 B/pixel), 17.4 (4), 25.6 (6),
// 33.8 KB (8); the dynamic part is the fp32 form's (12 480 B luminance ring + 13 056 B x Cd of watermark windows).  The worst case -- 8 B/pixel,
// full-resolution heat-map, Cd = 3 -- is 33 808 + 51 648 = 85 456 B of the CU's 163 840: ONE workgroup per CU (its 154 VGPRs would allow three
// waves per SIMD, so LDS binds there); every other combination stays below 80 KB (8 B/pixel: 72 976 B with Cd = 3 and no ring, 59 344 B with
// Cd = 1 and the ring) and runs two or more workgroups per CU.
template <class SF, bool JND, int CD>
__global__ __launch_bounds__(256) void embed_tail_rgb_stream_kernel(TailArgs a, JndTaps k, RgbGeo g, const int strip) {
  constexpr int BPP = SF::BPP, ROWB = SF::ROWB, NPR = SF::NPR, PPR = SF::PPR, ORB = TTW * BPP;
  constexpr int NLD = SG * NPR, NST = SG * PPR;
  constexpr int NLT = (NLD + 255) / 256, NOT = (NST + 255) / 256;               // pieces per thread and group, in and out
  static_assert(NLT <= 3 && NOT <= 2, "at most three pieces in and two out per thread and group");
  extern __shared__ float dyn_smem[];
  float* Lr = dyn_smem;                                        // [RING][TLW] luminance ring (JND only)
  float* DwB = dyn_smem + (JND ? RING * TLW : 0);              // [2][Cd][DW_H][DW_W] watermark source windows
  __shared__ __attribute__((aligned(16))) unsigned char Bst[2][SG * ROWB];         // incoming bytes of a group's four rows
  __shared__ __attribute__((aligned(16))) unsigned char Ost[2][SG * ORB];          // outgoing words
  __shared__ int ty_lo[2][SUBR], ty_n[2][SUBR], s_wy0[2];
  __shared__ float ty_w[2][SUBR][4];
  __shared__ int s_xhi, s_xlo;
  constexpr int dwsz = CD * DW_W * DW_H;
  const int x0 = blockIdx.x * TTW, y0 = blockIdx.y * strip, f = blockIdx.z;
  const int ys_end = min(a.H, y0 + strip);
  const int64_t rowb = (int64_t)a.W * BPP;
  const unsigned char* sbase = g.s.p + (int64_t)f * g.s.fs;
  unsigned char* dbase = const_cast<unsigned char*>(g.d.p) + (int64_t)f * g.d.fs;
  const int lx = threadIdx.x;
  const int x = x0 + lx;
  const bool xin = x < a.W;
  const int cx = xin ? x : a.W - 1;
  if (threadIdx.x == 0) s_xhi = 0;
  __syncthreads();
  const Taps tx = make_taps(cx, a.Sw, a.W, a.antialias);
  float wxs[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) wxs[j] = j < tx.n ? tap_w(tx, j) : 0.f;
  if (xin) atomicMax(&s_xhi, tx.lo + tx.n);
  if (threadIdx.x == 0) s_xlo = tx.lo;
  // halo columns of the luminance ring: threads 0 .. 3 carry one extra column each (x0 - 2, x0 - 1, x0 + 256, x0 + 257)
  const bool hal = JND && lx < 2 * HALO;
  const int hgx = lx < HALO ? x0 - HALO + lx : x0 + TTW + (lx - HALO);
  const int hl = lx < HALO ? lx : TTW + lx;
  const bool hin = hal && hgx >= 0 && hgx < a.W;

  // group gi brings rows y0 + 4 gi + 2 .. + 5: task lx + 256 i is piece (task % NPR) of row (task / NPR)
  struct Pieces { uint4 v[NLT]; };
  auto load_piece = [&](const int gi) __attribute__((always_inline)) -> Pieces {
    const int r0 = y0 + SG * gi + HALO;
    Pieces pc;
#pragma unroll
    for (int i = 0; i < NLT; ++i) {
      const int t = lx + 256 * i;
      pc.v[i] = uint4{0u, 0u, 0u, 0u};
      if (t < NLD) {
        const int lrow = t / NPR, lpc = t - lrow * NPR;
        const int gy = r0 + lrow;
        if (gy >= 0 && gy < a.H) pc.v[i] = SF::ld16(sbase + (int64_t)gy * g.s.pitch, (int64_t)x0 * BPP - 16 + 16 * lpc, rowb);
      }
    }
    return pc;
  };
  auto stash = [&](const int slot, const Pieces& pc) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NLT; ++i)
      if (lx + 256 * i < NLD) *reinterpret_cast<uint4*>(Bst[slot] + 16 * (lx + 256 * i)) = pc.v[i];
  };
  // the stored pixel of row q of the group in `slot` at tile column tc (-2 .. 257)
  auto stored = [&](const int slot, const int q, const int tc) __attribute__((always_inline)) -> Raw {
    return SF::from_lds(Bst[slot] + q * ROWB + 16 + tc * BPP);
  };
  Pieces pv = load_piece(-1);
  stash(0, pv);

  const KeyMix km = key_mix(a, f, CD);                   // value = wa*key[ka] + wb*key[kb]
  const float wa = km.wa, wb = km.wb;
  const float *dka = km.dka, *dkb = km.dkb, *hml = km.hml;
  const int splane = a.Sh * a.Sw;
  __syncthreads();                                             // s_xlo / s_xhi, byte stage of group -1
  const int wx0 = s_xlo, dww = s_xhi - s_xlo;

  auto stage = [&](const int sub, const int b) __attribute__((always_inline)) {      // source window + row taps of output rows [16 sub, 16 sub + 16)
    const int sy0 = y0 + SUBR * sub;
    const int lasty = min(SUBR, ys_end - sy0) - 1;
    int wy0, n0, wyl, nl;
    tap_range(sy0, a.Sh, a.H, a.antialias, wy0, n0);
    tap_range(sy0 + lasty, a.Sh, a.H, a.antialias, wyl, nl);
    const int dwh = wyl + nl - wy0;
    if (threadIdx.x < SUBR) {
      const int yy = sy0 + threadIdx.x;
      const Taps tp = make_taps(yy < a.H ? yy : a.H - 1, a.Sh, a.H, a.antialias);
      ty_lo[b][threadIdx.x] = tp.lo;
      ty_n[b][threadIdx.x] = tp.n;
#pragma unroll
      for (int j = 0; j < 4; ++j) ty_w[b][threadIdx.x][j] = j < tp.n ? tap_w(tp, j) : 0.f;
      if (threadIdx.x == 0) s_wy0[b] = wy0;
    }
    float* Dw = DwB + b * dwsz;
    const int nel = dwh * dww;
    for (int i0 = 0; i0 < nel; i0 += 4 * 256) {
      int sp[4], lo[4];
      float hmv[4], da[4][CD], db[4][CD];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = min(i0 + q * 256 + (int)threadIdx.x, nel - 1);
        const int yy = i / dww, xx = i - yy * dww;
        sp[q] = (wy0 + yy) * a.Sw + wx0 + xx;
        lo[q] = yy * DW_W + xx;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        hmv[q] = hml ? hml[sp[q]] : 1.f;
#pragma unroll
        for (int c = 0; c < CD; ++c) {
          da[q][c] = dka[c * splane + sp[q]];
          db[q][c] = wb != 0.f ? dkb[c * splane + sp[q]] : 0.f;
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (i0 + q * 256 + (int)threadIdx.x < nel) {
#pragma unroll
          for (int c = 0; c < CD; ++c) {
            float v = wa * da[q][c];
            if (wb != 0.f) v = __builtin_fmaf(wb, db[q][c], v);
            Dw[c * (DW_W * DW_H) + lo[q]] = hmv[q] * v;
          }
        }
    }
  };
  auto store_group = [&](const int gi) __attribute__((always_inline)) {         // words of output rows y0 + 4 gi .. + 3 -> the frame
#pragma unroll
    for (int i = 0; i < NOT; ++i) {
      const int t = lx + 256 * i;
      if (t < NST) {
        const int orow = t / PPR, pc = t - orow * PPR;
        const int y = y0 + SG * gi + orow;
        const int64_t off = (int64_t)x0 * BPP + 16 * pc;
        if (y < ys_end && off < rowb) SF::st16(dbase + (int64_t)y * g.d.pitch, off, rowb, Ost[gi & 1] + 16 * t);
      }
    }
  };

  const int nrows = ys_end - y0;
  const int niter = (nrows + SG - 1) / SG;
  float acc_la[2 * SG], acc_gx[2 * SG], acc_gy[2 * SG];
#pragma unroll
  for (int i = 0; i < 2 * SG; ++i) { acc_la[i] = 0.f; acc_gx[i] = 0.f; acc_gy[i] = 0.f; }
  float hist[2][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
  Raw hraw[2] = {{0u, 0u}, {0u, 0u}};
  pv = load_piece(0);
  stage(0, 0);
  for (int it = -1; it < niter; ++it) {
    const int r0 = y0 + SG * it + HALO;                       // first incoming row of this group; its output rows are r0 - 2 .. r0 + 1
    const int slot0 = ((it + 1) % 3) * SG;
    const int bs = (it + 1) & 1;
    float cu[SG][3];
    Raw craw[SG];
#pragma unroll
    for (int q = 0; q < SG; ++q) {
      craw[q] = stored(bs, q, lx);
      SF::decode(craw[q], g.pos, cu[q]);
    }
    if (JND) {
#pragma unroll
      for (int q = 0; q < SG; ++q) {
        const int gy = r0 + q;
        const bool rok = gy >= 0 && gy < a.H;
        Lr[(slot0 + q) * TLW + lx + HALO] = (rok && xin) ? lum255(cu[q][0], cu[q][1], cu[q][2]) : 0.f;
        if (hal) {
          float hp[3];
          SF::decode(stored(bs, q, hl - HALO), g.pos, hp);
          Lr[(slot0 + q) * TLW + hl] = (rok && hin) ? lum255(hp[0], hp[1], hp[2]) : 0.f;
        }
      }
    }
    if (it + 1 < niter) {
      stash(bs ^ 1, pv);                                                    // group it + 1, read after the barrier below
      if (it + 2 < niter) pv = load_piece(it + 2);                          // in flight for a whole group
      if (((it + 1) & 3) == 0 && it + 1 > 0) stage((it + 1) >> 2, ((it + 1) >> 2) & 1);
    }
    __syncthreads();
    if (it >= 1) store_group(it - 1);
    const int sb = (it >> 2) & 1;
    const float* Dw = DwB + sb * dwsz;
    unsigned char* Og = Ost[it & 1];
#pragma unroll
    for (int j = 0; j < SG; ++j) {
      if (JND) {
        const float* row = Lr + (slot0 + j) * TLW + lx + HALO;
        const float m2 = row[-2], m1 = row[-1], c0 = row[0], p1 = row[1], p2 = row[2];
        const float h3 = m1 + c0 + p1;
        const float h5 = h3 + m2 + p2;
        const float sd = p1 - m1;
        const float tt = m1 + 2.f * c0 + p1;
#pragma unroll
        for (int i = j; i <= j + 4; ++i) {
          const int dy = 2 + j - i;                            // incoming row - output row
          if (dy >= -2 && dy <= 2) acc_la[i] += h5;
          if (dy >= -1 && dy <= 1) acc_la[i] += h3;
          if (dy == 0) acc_la[i] -= 2.f * c0;
          if (dy == -1 || dy == 1) acc_gx[i] += sd;
          if (dy == 0) acc_gx[i] += 2.f * sd;
          if (dy == -1) acc_gy[i] += tt;
          if (dy == 1) acc_gy[i] -= tt;
        }
      }
      const int y = r0 - HALO + j;                             // the output row this incoming row completes
      if (it >= 0 && y < ys_end && xin) {
        float hm = 1.f;
        if (JND) {
          if (fabsf(acc_la[j] * (1.f / 32.f) - 127.f) < 0.02f) hm = jnd_at_ring(Lr, (slot0 + j + RING - HALO) % RING, lx + HALO, k);
          else hm = jnd_finish(acc_la[j], acc_gx[j], acc_gy[j]);
        }
        const int ly = (SG * it + j) & (SUBR - 1);
        float d[3] = {0.f, 0.f, 0.f};
        const int basep = (ty_lo[sb][ly] - s_wy0[sb]) * DW_W + (tx.lo - wx0);
        tail_taps<3, DW_H>(d, Dw, CD, basep, tx.n, ty_n[sb][ly], wxs, ty_w[sb][ly]);
        if (JND)
#pragma unroll
          for (int c = 0; c < CD; ++c) d[c] = hm * d[c];
        float v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float p = j < 2 ? hist[j][c] : cu[j - 2][c];
          const float t = blend_px(a.scaling_i, a.scaling_w, p, d[CD == 1 ? 0 : c], hm, false);
          v[c] = t <= 0.f ? 0.f : (t >= 1.f ? 1.f : t);
        }
        SF::to_lds(Og + j * ORB + lx * BPP, SF::encode(j < 2 ? hraw[j] : craw[j - 2], g.pos, v));
      }
    }
#pragma unroll
    for (int i = 0; i < SG; ++i) {
      acc_la[i] = acc_la[i + SG]; acc_gx[i] = acc_gx[i + SG]; acc_gy[i] = acc_gy[i + SG];
      acc_la[i + SG] = 0.f; acc_gx[i + SG] = 0.f; acc_gy[i + SG] = 0.f;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) { hist[0][c] = cu[2][c]; hist[1][c] = cu[3][c]; }
    hraw[0] = craw[2]; hraw[1] = craw[3];
  }
  __syncthreads();
  store_group(niter - 1);
}

}  // namespace
