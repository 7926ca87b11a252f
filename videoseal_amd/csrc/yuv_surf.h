// YUV frames as a decoder delivers them: vs_resize_pre and vs_embed_tail (shell.hip) with the colour conversion fused in, each way.  Four
// kernels (resize and tail, each as a tile form and a row-streaming form), one body per kernel, a surface trait per format.  This header holds
// the trait, the kernel bodies and their launchers; yuv420.hip instantiates the 4:2:0 traits, yuv4xx.hip the 4:2:2 and 4:4:4 ones, yuv_clips.hip
// the list forms of three of the kernels (lists of clips: the same bodies behind another prologue, see "Where a workgroup works" below).
//   nv12       uint8   Y plane + interleaved CbCr plane           i420       uint8   Y, U, V planes
//   p010       uint16  as nv12, code = word >> 6                  yuv420p10  uint16  as i420, code = min(word, 1023)
//   nv16 / p210: as nv12 / p010 with a chroma row per luma row;  yuv422p / yuv422p10: as i420 / yuv420p10 with a chroma row per luma row;
//   yuv444p / yuv444p10: three planes of H x W.
// The chroma geometry is the pair of subsampling shifts (SX, SY): (1, 1) for 4:2:0, (1, 0) for 4:2:2, (0, 0) for 4:4:4.  A chroma block is
// (1 << SX) x (1 << SY) pixels: every pixel of a block uses the block's (Cb, Cr), the block's output chroma is the mean of its per-pixel values.
// Every plane has its own row pitch and frame stride in bytes (any value, odd ones included).  The colour affines come from the host in code
// units of the surface's depth (videoseal_amd/yuv420.py); RGB is clamped to [0, 1] after decoding; output codes are
// floor(clamp(v, 0, 2^depth - 1) + 0.5), the chroma of a block is the mean of its per-pixel values, rounded once.
// The trait supplies "load 16 bytes of this row of this plane" (8 or 16 samples; a subsampled planar chroma piece serves twice as many luma columns),
// "sample q as a float code" and "store 16 bytes"; a piece moves as one 16-byte access where it lies inside the row and its address is
// aligned, sample by sample, guarded, elsewhere -- padding bytes are neither used nor written.  Conversion, filter taps, JND and blend are the
// same expressions in the same order for every trait (shell_common.h), so layouts that hold the same codes give the same bits.
#pragma once
#include "tail_phases.h"

#include <type_traits>

namespace {

struct YuvSurf { const unsigned char* p[3]; int64_t pitch[3], fs[3]; };       // bytes
struct YuvGeo { YuvSurf s, d; Nv12Mat dec, enc; };

// The sample codec of a surface: stored word <-> sample value, sample triple <-> RGB.  For the YUV formats a sample is an integer code and the
// colour affines stand between codes and RGB; half_surf.h puts floating-point samples (and no matrix) behind the same four functions.
template <int DEPTH_, bool MSB_>
struct YuvCodec {
  static constexpr int BPS = DEPTH_ > 8 ? 2 : 1;            // bytes per sample
  using S = typename std::conditional<BPS == 2, unsigned short, unsigned char>::type;
  static __device__ __forceinline__ float val(const unsigned raw) {            // stored word -> code
    if (BPS == 1) return (float)raw;
    return MSB_ ? (float)(raw >> 6) : (float)(raw < 1023u ? raw : 1023u);
  }
  static __device__ __forceinline__ S word(const float v) {                    // code value -> stored word, the one rounding
    const int c = (int)floorf(fminf(fmaxf(v, 0.f), (float)((1 << DEPTH_) - 1)) + 0.5f);
    return (S)(BPS == 2 && MSB_ ? c << 6 : c);
  }
  static __device__ __forceinline__ void rgb(const Nv12Mat& k, const float y, const float cb, const float cr, float (&out)[3]) { nv12_rgb(k, y, cb, cr, out); }
  static __device__ __forceinline__ float aff(const Nv12Mat& k, const int r, const float a, const float b, const float c) { return nv12_aff(k, r, a, b, c); }
};

template <bool PLANAR_, int DEPTH_, bool MSB_, int SX_ = 1, int SY_ = 1, class CODEC_ = YuvCodec<DEPTH_, MSB_>>
struct Surf {
  static_assert((SX_ == 1 && (SY_ == 0 || SY_ == 1)) || (SX_ == 0 && SY_ == 0 && PLANAR_), "4:2:0, 4:2:2, or planar 4:4:4");
  static constexpr bool PLANAR = PLANAR_;
  static constexpr int DEPTH = DEPTH_;
  static constexpr int SX = SX_, SY = SY_;                  // chroma subsampling shifts: a chroma sample serves (1 << SX) x (1 << SY) pixels
  static constexpr bool PSUB = PLANAR_ && SX_ == 1;         // planar chroma of half width: a piece serves 2 SPP luma columns
  static constexpr int BPS = CODEC_::BPS;                   // bytes per sample
  static constexpr int SPP = 16 / BPS;                      // samples per 16-byte piece
  static constexpr int NL = PSUB ? 2 : 1;                   // luma pieces per row of a resize chunk
  static constexpr int CW = NL * SPP;                       // luma columns of a resize chunk: one chroma piece per plane and chroma row serves them
  static constexpr int NCR = SY_ ? 1 : 2;                   // chroma rows of a row pair
  static constexpr int NCP = PLANAR_ && !SX_ ? 2 : 1;       // chroma pieces a row-streaming resize task loads per chroma row (4:4:4: its own U and V)
  static constexpr int PCP = (130 + 2 * SPP - 1) / SPP;     // pieces of a half-width planar chroma row of the tail window: chroma columns x0/2 - SPP .. x0/2 + 129
  static constexpr int NVW = TTW + 2 * SPP;                 // tail window: luma columns x0 - SPP .. x0 + 255 + SPP
  static constexpr int NPY = NVW / SPP;                     // its pieces per luma row
  static constexpr int NPP = PSUB ? PCP : NPY;              // pieces of one planar chroma plane's row of the window (4:4:4: the luma window's columns)
  static constexpr int NPC = PLANAR_ ? 2 * NPP : NPY;       // ... per chroma row (planar: U pieces, then V pieces)
  static constexpr int CRS = NPC * SPP;                     // samples of a chroma row in LDS
  static constexpr int PPR = TTW / SPP;                     // pieces of an output row of 256 columns
  static constexpr int OCW = PLANAR_ && !SX_ ? 2 * TTW : TTW;   // samples of an output chroma row of a tile: pairs, U then V halves, or (4:4:4) 256 of U then 256 of V
  static constexpr int OPC = OCW / SPP;                     // its pieces
  using S = typename CODEC_::S;
  static __host__ __device__ __forceinline__ int crows(const int H) { return SY_ ? H >> 1 : H; }      // rows of a chroma plane
  static __host__ __device__ __forceinline__ int pcols(const int W) { return SX_ ? W >> 1 : W; }      // samples of a planar chroma row

  static __device__ __forceinline__ float val(const unsigned raw) { return CODEC_::val(raw); }
  static __device__ __forceinline__ S word(const float v) { return CODEC_::word(v); }
  static __device__ __forceinline__ void rgb(const Nv12Mat& k, const float y, const float cb, const float cr, float (&out)[3]) { CODEC_::rgb(k, y, cb, cr, out); }
  static __device__ __forceinline__ float aff(const Nv12Mat& k, const int r, const float a, const float b, const float c) { return CODEC_::aff(k, r, a, b, c); }
  static __device__ __forceinline__ unsigned gld(const unsigned char* __restrict__ row, const int col) {      // one sample, any address
    if (BPS == 1) return row[col];
    return (unsigned)row[2 * col] | ((unsigned)row[2 * col + 1] << 8);
  }
  // 16 bytes = SPP samples from sample column `col` of a row of W samples; samples outside the row read as zero
  static __device__ __forceinline__ uint4 ld16(const unsigned char* __restrict__ row, const int col, const int W) {
    const unsigned char* p = row + (int64_t)col * BPS;
    if (col >= 0 && col + SPP <= W && (reinterpret_cast<uintptr_t>(p) & 15) == 0) return *reinterpret_cast<const uint4*>(p);
    unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int q = 0; q < SPP; ++q) {
      const int c = col + q;
      if (c >= 0 && c < W) {
        if (BPS == 1) w[q >> 2] |= (unsigned)p[q] << (8 * (q & 3));
        else w[q >> 1] |= ((unsigned)p[2 * q] | ((unsigned)p[2 * q + 1] << 8)) << (16 * (q & 1));
      }
    }
    return uint4{w[0], w[1], w[2], w[3]};
  }
  static __device__ __forceinline__ void st16(unsigned char* __restrict__ row, const int col, const int W, const S* __restrict__ lds) {
    unsigned char* p = row + (int64_t)col * BPS;
    if (col + SPP <= W && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
      *reinterpret_cast<uint4*>(p) = *reinterpret_cast<const uint4*>(lds);
      return;
    }
    for (int q = 0; q < SPP; ++q)
      if (col + q < W) {
        if (BPS == 1) {
          p[q] = (unsigned char)lds[q];
        } else {
          p[2 * q] = (unsigned char)(lds[q] & 0xff);
          p[2 * q + 1] = (unsigned char)(lds[q] >> 8);
        }
      }
  }
  static __device__ __forceinline__ unsigned raw(const uint4& v, const int q) {       // q: compile-time constant after unrolling
    if (BPS == 1) {
      const unsigned w = q < 4 ? v.x : (q < 8 ? v.y : (q < 12 ? v.z : v.w));
      return (w >> (8 * (q & 3))) & 0xffu;
    }
    const unsigned w = q < 2 ? v.x : (q < 4 ? v.y : (q < 6 ? v.z : v.w));
    return (w >> (16 * (q & 1))) & 0xffffu;
  }
  // chroma of luma column xx straight from the frame (the unstaged paths of the resize tile kernel)
  static __device__ __forceinline__ void gchroma(const unsigned char* __restrict__ u, const unsigned char* __restrict__ v, const int xx,
                                                 float& cb, float& cr) {
    if (PLANAR_) { cb = val(gld(u, xx >> SX_)); cr = val(gld(v, xx >> SX_)); }
    else { cb = val(gld(u, xx & ~1)); cr = val(gld(u, xx | 1)); }
  }
  // chroma of window luma column wc (frame column x0 - SPP + wc) from a chroma row staged by the tail kernels
  static __device__ __forceinline__ void lchroma(const S* __restrict__ crow, const int wc, float& cb, float& cr) {
    if (PSUB) { cb = val(crow[(wc + SPP) >> 1]); cr = val(crow[PCP * SPP + ((wc + SPP) >> 1)]); }
    else if (PLANAR_) { cb = val(crow[wc]); cr = val(crow[NVW + wc]); }
    else { cb = val(crow[wc & ~1]); cr = val(crow[wc | 1]); }
  }
  // piece p of a chroma row of the tail window: plane, first sample column and row width for ld16
  static __device__ __forceinline__ void cpiece(const int p, const int x0, const int W, int& pl, int& col, int& cw) {
    if (PSUB) { pl = p < PCP ? 1 : 2; col = x0 / 2 - SPP + SPP * (p < PCP ? p : p - PCP); cw = W >> 1; }
    else if (PLANAR_) { pl = p < NPY ? 1 : 2; col = x0 - SPP + SPP * (p < NPY ? p : p - NPY); cw = W; }
    else { pl = 1; col = x0 - SPP + SPP * p; cw = W; }
  }
  // piece pc of an output chroma row (OCW samples: interleaved pairs, 128 of U then 128 of V, or 256 of U then 256 of V)
  static __device__ __forceinline__ void opiece(const int pc, const int x0, const int W, int& pl, int& col, int& cw) {
    if (PSUB) { const int hv = pc >= PPR / 2 ? 1 : 0; pl = 1 + hv; col = x0 / 2 + SPP * (pc - hv * (PPR / 2)); cw = W >> 1; }
    else if (PLANAR_) { const int hv = pc >= PPR ? 1 : 0; pl = 1 + hv; col = x0 + SPP * (pc - hv * PPR); cw = W; }
    else { pl = 1; col = x0 + SPP * pc; cw = W; }
  }
  // where lane lx leaves the block's chroma code in an output chroma row (SX = 1): even lanes hold Cb, odd lanes Cr
  static __device__ __forceinline__ int ocol(const int lx) { return PLANAR_ ? ((lx & 1) ? TTW / 2 : 0) + (lx >> 1) : lx; }
  // The chroma of one output row's pixel, reduced over its block and left in the tile's output chroma row `crow`.  cbs / crs hold the sums
  // over the block's rows of this lane's column; with SX = 1 the other column comes from the neighbouring lane (every lane of a pair calls
  // this together), the even lane stores Cb and the odd lane Cr.  4:4:4: the lane stores both, its own values.
  static __device__ __forceinline__ void ochroma(S* __restrict__ crow, const int lx, const bool live, float cbs, float crs) {
    if (SX_) {
      cbs += __shfl_xor(cbs, 1);
      crs += __shfl_xor(crs, 1);
      if (live) crow[ocol(lx)] = word((SY_ ? 0.25f : 0.5f) * ((lx & 1) ? crs : cbs));
    } else if (live) {
      crow[lx] = word(cbs);
      crow[TTW + lx] = word(crs);
    }
  }

  // the pieces of CW luma columns x one row pair: 2 NL luma pieces and the chroma they use (one chroma row, or with SY = 0 one per luma row).
  // A row past the last one (odd H) is not read: its pieces are zero and nobody uses them.
  struct Chunk {
    uint4 y[2][NL];
    uint4 c[NCR][2];
    __device__ __forceinline__ void load(const unsigned char* yb, const int64_t yp, const unsigned char* ub, const int64_t up,
                                         const unsigned char* vb, const int64_t vp, const int row, const int col, const int H, const int W) {
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < NL; ++i)
          y[h][i] = (SY_ || row + h < H) ? ld16(yb + (int64_t)(row + h) * yp, col + SPP * i, W) : uint4{0u, 0u, 0u, 0u};       // (SY = 1: H is even)
#pragma unroll
      for (int h = 0; h < NCR; ++h) {
        const int cy = SY_ ? row >> 1 : row + h;
        c[h][0] = c[h][1] = uint4{0u, 0u, 0u, 0u};
        if (SY_ || cy < H) {
          if (PLANAR_) {
            c[h][0] = ld16(ub + (int64_t)cy * up, col >> SX_, pcols(W));
            c[h][1] = ld16(vb + (int64_t)cy * vp, col >> SX_, pcols(W));
          } else {
            c[h][0] = ld16(ub + (int64_t)cy * up, col, W);
          }
        }
      }
    }
    __device__ __forceinline__ float lum(const int h, const int q) const { return val(raw(y[h][q / SPP], q % SPP)); }
    __device__ __forceinline__ float cb(const int h, const int q) const { return PLANAR_ ? val(raw(c[h % NCR][0], q >> SX_)) : val(raw(c[h % NCR][0], q & ~1)); }
    __device__ __forceinline__ float cr(const int h, const int q) const { return PLANAR_ ? val(raw(c[h % NCR][1], q >> SX_)) : val(raw(c[h % NCR][0], q | 1)); }
  };
  // the pieces of SPP luma columns x one row pair for the row-streaming resize: two luma pieces and, per chroma row, ONE chroma piece (4:4:4:
  // two, its own U and V).  Half-width planar chroma: the lanes of a pair hold neighbouring chunks; the even lane loads the U piece that
  // serves both, the odd lane the V piece, and each hands the other the half it needs when the chunk is converted (one 16-byte load of U and
  // one of V per 2 SPP luma columns and chroma row, as many loads per thread as for an interleaved surface).  A 4:4:4 piece serves exactly its
  // own SPP columns: nothing is shared and nothing crosses lanes.
  struct SChunk {
    uint4 y[2];
    uint4 c[NCR][NCP];
    __device__ __forceinline__ void zero() {
      y[0] = y[1] = uint4{0u, 0u, 0u, 0u};
#pragma unroll
      for (int h = 0; h < NCR; ++h)
#pragma unroll
        for (int i = 0; i < NCP; ++i) c[h][i] = uint4{0u, 0u, 0u, 0u};
    }
    // (zero() first: a row past the last one -- odd H -- is not read)
    __device__ __forceinline__ void load(const unsigned char* yb, const int64_t yp, const unsigned char* ub, const int64_t up,
                                         const unsigned char* vb, const int64_t vp, const int row, const int col, const int H, const int W, const bool odd) {
#pragma unroll
      for (int h = 0; h < 2; ++h)
        if (SY_ || row + h < H) y[h] = ld16(yb + (int64_t)(row + h) * yp, col, W);
#pragma unroll
      for (int h = 0; h < NCR; ++h) {
        const int cy = SY_ ? row >> 1 : row + h;
        if (SY_ || cy < H) {
          if (PSUB) c[h][0] = odd ? ld16(vb + (int64_t)cy * vp, (col - SPP) >> 1, W >> 1) : ld16(ub + (int64_t)cy * up, col >> 1, W >> 1);
          else if (PLANAR_) { c[h][0] = ld16(ub + (int64_t)cy * up, col, W); c[h][NCP - 1] = ld16(vb + (int64_t)cy * vp, col, W); }
          else c[h][0] = ld16(ub + (int64_t)cy * up, col, W);
        }
      }
    }
    // the U and V (or CbCr) pieces of chroma row h  (every lane of a pair calls this together)
    __device__ __forceinline__ void chroma(const int h, const bool odd, uint4& cu, uint4& cv) const {
      if (PSUB) {
        const uint4& p = c[h][0];
        const unsigned r0 = __shfl_xor(odd ? p.x : p.z, 1), r1 = __shfl_xor(odd ? p.y : p.w, 1);
        cu = odd ? uint4{r0, r1, 0u, 0u} : uint4{p.x, p.y, 0u, 0u};
        cv = odd ? uint4{p.z, p.w, 0u, 0u} : uint4{r0, r1, 0u, 0u};
      } else {
        cu = c[h][0];
        cv = c[h][NCP - 1];
      }
    }
    __device__ __forceinline__ float lum(const int h, const int q) const { return val(raw(y[h], q)); }
    static __device__ __forceinline__ float cb(const uint4& cu, const int q) { return PLANAR_ ? val(raw(cu, q >> SX_)) : val(raw(cu, q & ~1)); }
    static __device__ __forceinline__ float cr(const uint4& cv, const int q) { return PLANAR_ ? val(raw(cv, q >> SX_)) : val(raw(cv, q | 1)); }
  };
};

// ---- Where a workgroup works: the prologue of the three kernels that have a list form (the two tile kernels and the row-streaming resize).
// Grid form: the launch has ONE surface; blockIdx.{x, y, z} are (tile column, tile row, frame) and H, W, the destinations and the tail's
// arguments are the launch's.  List form (vs_resize_pre_yuv_clips / vs_embed_tail_yuv_clips, videoseal_yuv_clips.h): the launch is a flat
// grid over at most VS_YUV_CLIPS_PER_LAUNCH slots whose descriptors and prefix table of first workgroups travel in the kernel arguments; a
// workgroup finds its slot by the halving search of images_find (shell.hip) -- four steps -- and (frame, tile row, tile column) as clips_item
// does, frame-major.  Everything it finds is workgroup-uniform: scalar loads and scalar compares, the slot's pointers and sizes stay in SGPRs.
// The body sees a slot as a clip of its own: dst_rgb / hmap_lowres moved to the slot's first frame, dst_key / delta to its first key frame,
// total_key = ceil(F / step).  The kernels take the source (and the tail's geometry) as a template parameter and ask the overloads below;
// for the grid form every one of them is the identity, so the grid instantiations compile to the instructions they had before the list
// forms existed, and the statements after the prologue are one text for both.
constexpr int YUV_CLIPS = 16;      // VS_YUV_CLIPS_PER_LAUNCH (yuv_clips.hip holds the two together)
struct YuvClipSlot { YuvSurf s, d; int F, H, W, first_frame, first_key, cols, tiles, pad_; };      // cols: tiles per tile row; tiles: per frame
struct YuvClipsArgs {
  int first_wg[YUV_CLIPS + 1];       // entries past the launch's slot count hold the grid size: never reached by a workgroup
  int pad_;
  YuvClipSlot slot[YUV_CLIPS];
};
struct YuvClipsGeo { YuvClipsArgs c; Nv12Mat dec, enc; };
struct YuvGeoRef { const YuvSurf& s; const YuvSurf& d; const Nv12Mat& dec; const Nv12Mat& enc; };      // a slot's YuvGeo, in place

struct YuvAt { int k, f; unsigned bx, by; };       // slot, frame of the slot, tile column, tile row (unsigned, as blockIdx is: x0 = bx * TTW is the grid form's expression)
__device__ __forceinline__ YuvAt yuv_at(const YuvSurf&) { return YuvAt{0, (int)blockIdx.z, blockIdx.x, blockIdx.y}; }
__device__ __forceinline__ YuvAt yuv_at(const YuvGeo&) { return YuvAt{0, (int)blockIdx.z, blockIdx.x, blockIdx.y}; }
__device__ __forceinline__ YuvAt yuv_at(const YuvClipsArgs& g) {
  const int wg = blockIdx.x;
  int k = 0;
#pragma unroll
  for (int s = YUV_CLIPS / 2; s >= 1; s >>= 1)
    if (wg >= g.first_wg[k + s]) k += s;
  const int t = wg - g.first_wg[k];
  const int tiles = g.slot[k].tiles, cols = g.slot[k].cols;
  const int f = t / tiles;
  const int r = t - f * tiles;
  const int by = r / cols;
  return YuvAt{k, f, (unsigned)(r - by * cols), (unsigned)by};
}
__device__ __forceinline__ YuvAt yuv_at(const YuvClipsGeo& g) { return yuv_at(g.c); }
__device__ __forceinline__ const YuvSurf& yuv_src(const YuvSurf& s, const int) { return s; }
__device__ __forceinline__ const YuvSurf& yuv_src(const YuvClipsArgs& g, const int k) { return g.slot[k].s; }
__device__ __forceinline__ int yuv_h(const YuvSurf&, const int, const int H) { return H; }
__device__ __forceinline__ int yuv_h(const YuvClipsArgs& g, const int k, const int) { return g.slot[k].H; }
__device__ __forceinline__ int yuv_w(const YuvSurf&, const int, const int W) { return W; }
__device__ __forceinline__ int yuv_w(const YuvClipsArgs& g, const int k, const int) { return g.slot[k].W; }
// the resize's destinations, moved to the slot's first frame / first key frame (frame: oh x ow x 4 floats)
__device__ __forceinline__ float* yuv_rgb_at(const YuvSurf&, const int, float* p, const int, const int) { return p; }
__device__ __forceinline__ float* yuv_rgb_at(const YuvClipsArgs& g, const int k, float* p, const int oh, const int ow) {
  return p ? p + g.slot[k].first_frame * ((int64_t)oh * ow * 4) : nullptr;
}
__device__ __forceinline__ float* yuv_key_at(const YuvSurf&, const int, float* p, const int, const int) { return p; }
__device__ __forceinline__ float* yuv_key_at(const YuvClipsArgs& g, const int k, float* p, const int oh, const int ow) {
  return p ? p + g.slot[k].first_key * ((int64_t)oh * ow * 4) : nullptr;
}
// the tail's arguments and geometry of the slot (as embed_tail_clips_kernel of shell.hip sets them)
__device__ __forceinline__ void yuv_tail_args(const YuvGeo&, const int, TailArgs&) {}
__device__ __forceinline__ void yuv_tail_args(const YuvClipsGeo& g, const int k, TailArgs& a) {
  a.F = g.c.slot[k].F;
  a.H = g.c.slot[k].H;
  a.W = g.c.slot[k].W;
  a.total_key = (a.F + a.step - 1) / a.step;
  const int64_t splane = (int64_t)a.Sh * a.Sw;
  a.delta += g.c.slot[k].first_key * splane * a.Cd;
  if (a.hmap_lowres) a.hmap_lowres += g.c.slot[k].first_frame * splane;
}
__device__ __forceinline__ const YuvGeo& yuv_geo(const YuvGeo& g, const int) { return g; }
__device__ __forceinline__ YuvGeoRef yuv_geo(const YuvClipsGeo& g, const int k) { return YuvGeoRef{g.c.slot[k].s, g.c.slot[k].d, g.dec, g.enc}; }

// Tile form of the resize: resize_pre_kernel (shell.hip) on YUV frames -- conversion and clamp per source pixel in front of the filter, then
// the same taps in the same order.  A workgroup owns 32 x 8 output pixels.  Staging: a task is one chunk of CW columns x one row PAIR (the luma
// pieces of both rows and the chroma they share), converted from registers into the fp32 window in LDS; the window of at most RS_WW x RS_WH
// pixels spans <= 15 chunks x 17 pairs, tasks taken in turn by the 256 threads.  A window that does not fit is filtered straight from the frame.
// SRC: YuvSurf (grid form) or YuvClipsArgs (list form: B, H_ and W_ are not used, the destinations are the whole tensors).
template <class SF, class SRC = YuvSurf>
__global__ __launch_bounds__(256) void resize_pre_yuv_kernel(SRC src, Nv12Mat dec, int B, int H_, int W_, int oh, int ow, int antialias,
                                                             float* __restrict__ dst_rgb_, float mul, float add, float* __restrict__ dst_key_,
                                                             int key_step, int key_mode, float y0, float y1, float y2) {
  __shared__ float Lw[3 * RS_WH * RS_WW];
  constexpr int CW = SF::CW;
  const YuvAt at = yuv_at(src);
  const YuvSurf& s = yuv_src(src, at.k);
  const int H = yuv_h(src, at.k, H_), W = yuv_w(src, at.k, W_);
  float* __restrict__ dst_rgb = yuv_rgb_at(src, at.k, dst_rgb_, oh, ow);
  float* __restrict__ dst_key = yuv_key_at(src, at.k, dst_key_, oh, ow);
  const int ox0 = at.bx * 32, oy0 = at.by * 8;
  const int b = at.f;
  const unsigned char* base = s.p[0] + (int64_t)b * s.fs[0];
  const unsigned char* ubase = s.p[1] + (int64_t)b * s.fs[1];
  const unsigned char* vbase = SF::PLANAR ? s.p[2] + (int64_t)b * s.fs[2] : ubase;
  const int64_t pitch = s.pitch[0], upitch = s.pitch[1], vpitch = SF::PLANAR ? s.pitch[2] : s.pitch[1];
  int x_lo, y_lo, x_hi, y_hi, n_;
  tap_range(ox0, W, ow, antialias, x_lo, n_);
  tap_range(min(ox0 + 31, ow - 1), W, ow, antialias, x_hi, n_);
  const int ww = x_hi + n_ - x_lo;
  tap_range(oy0, H, oh, antialias, y_lo, n_);
  tap_range(min(oy0 + 7, oh - 1), H, oh, antialias, y_hi, n_);
  const int wh = y_hi + n_ - y_lo;
  const bool staged = ww <= RS_WW && wh <= RS_WH;          // block-uniform
  if (staged) {
    const int pc0 = x_lo / CW, npc = ((x_lo + ww - 1) / CW) - pc0 + 1;
    const int rp0 = y_lo >> 1, nrp = ((y_lo + wh - 1) >> 1) - rp0 + 1;
    for (int t = threadIdx.x; t < npc * nrp; t += 256) {
      const int ri = t / npc, pi = t - ri * npc;
      const int col = (pc0 + pi) * CW, row = (rp0 + ri) * 2;            // row + 1 < H where H is even; the chunk reads no row >= H
      typename SF::Chunk ch;
      ch.load(base, pitch, ubase, upitch, vbase, vpitch, row, col, H, W);
#pragma unroll
      for (int q = 0; q < CW; ++q) {
        const int xx = col + q - x_lo;
        if (xx >= 0 && xx < ww) {
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int yy = row + h - y_lo;
            if (yy >= 0 && yy < wh) {                                   // (the window ends inside the frame: yy < wh => row + h < H)
              float rgb[3];
              SF::rgb(dec, ch.lum(h, q), ch.cb(h, q), ch.cr(h, q), rgb);
#pragma unroll
              for (int c = 0; c < 3; ++c) Lw[(c * RS_WH + yy) * RS_WW + xx] = rgb[c];
            }
          }
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
      const int yy = ty.lo + jy;
      const unsigned char* yr = base + (int64_t)yy * pitch;
      const unsigned char* ur = ubase + (int64_t)(yy >> SF::SY) * upitch;
      const unsigned char* vr = vbase + (int64_t)(yy >> SF::SY) * vpitch;
      CompSum r3[3];
      for (int jx = 0; jx < tx.n; ++jx) {
        const float wx = tap_w(tx, jx);
        const int xx = tx.lo + jx;
        float rgb[3], cb, cr;
        SF::gchroma(ur, vr, xx, cb, cr);
        SF::rgb(dec, SF::val(SF::gld(yr, xx)), cb, cr, rgb);
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
      const int yy = ty.lo + jy;
      const unsigned char* yr = base + (int64_t)yy * pitch;
      const unsigned char* ur = ubase + (int64_t)(yy >> SF::SY) * upitch;
      const unsigned char* vr = vbase + (int64_t)(yy >> SF::SY) * vpitch;
      float r[3] = {0.f, 0.f, 0.f};
      for (int jx = 0; jx < tx.n; ++jx) {
        const float wx = tap_w(tx, jx);
        const int xx = tx.lo + jx;
        float rgb[3], cb, cr;
        SF::gchroma(ur, vr, xx, cb, cr);
        SF::rgb(dec, SF::val(SF::gld(yr, xx)), cb, cr, rgb);
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

// Row-streaming form of the resize: the structure of vs_rs::resize_stream_tile (resize_stream.h) with another loader (see the note there).  A workgroup owns OW output columns x a
// strip of output rows and walks the input rows eight at a time, groups starting on an EVEN row: a group is four row pairs.  The window starts
// on a multiple of `align` = max(16, Surf::CW) columns (luma and chroma pieces stay 16-byte aligned); a load task is one piece of SPP columns
// x one row pair of the group's four (Surf::SChunk: two luma pieces and one chroma piece -- with SY = 0 one per row of the pair, for 4:4:4 a U
// and a V piece per row -- requested one group ahead), <= 56 pieces x 4 pairs; planar surfaces of half-width chroma take an even number of
// pieces per row, so that the lanes of a pair share a chroma piece.  With an odd H the last pair has one row.  Every luma row and every chroma
// row is fetched once per column tile (+ the first window of a strip).  The thread that holds a task converts its pixels straight from
// registers into the [8][3][INW] fp32 window; the horizontal and vertical passes, their expressions and their order are resize_stream_body's
// and the tile kernel's: the same bits.
template <class SF> constexpr int yuv_rs_align() { return SF::CW > 16 ? SF::CW : 16; }      // window start, in columns: the margin of vs_rs::rs_pick
template <class SF, int OW, class SRC = YuvSurf>
__global__ __launch_bounds__(256) void resize_pre_yuv_stream_kernel(SRC src, Nv12Mat dec, int H_, int W_, int oh, int ow, int antialias,
                                                                    ResizePreEpi epi, int strip) {
  using namespace vs_rs;
  extern __shared__ __attribute__((aligned(16))) float rs_smem[];
  constexpr int INW = RsGeo<OW>::INW, MT = RsGeo<OW>::MT, RING = RsGeo<OW>::RING, NPART = 256 / OW, RPP = RS_GI / NPART;
  constexpr int CW = SF::SPP, ALIGN = yuv_rs_align<SF>();
  static_assert(INW % (2 * CW) == 0 && 4 * (INW / CW) <= 256, "a piece (and a pair of them) ends inside the window row; one load task per thread");
  float* In = rs_smem;                                   // [RS_GI][3][INW]
  float* Hr = rs_smem + RS_GI * 3 * INW;                 // [RING][3][OW]
  float* Wy = Hr + RING * 3 * OW;                        // [RS_WTAB_ROWS][MT] vertical weights | first row | tap count
  int* WyLo = reinterpret_cast<int*>(Wy + RS_WTAB_ROWS * MT);
  int* WyN = WyLo + RS_WTAB_ROWS;
  const YuvAt at = yuv_at(src);
  const YuvSurf& s = yuv_src(src, at.k);
  const int H = yuv_h(src, at.k, H_), W = yuv_w(src, at.k, W_);
  epi.dst_rgb = yuv_rgb_at(src, at.k, epi.dst_rgb, oh, ow);
  epi.dst_key = yuv_key_at(src, at.k, epi.dst_key, oh, ow);
  const int ox0 = at.bx * OW, oy0 = at.by * strip, b = at.f;
  const int oy_end = min(oh, oy0 + strip);
  const unsigned char* base = s.p[0] + (int64_t)b * s.fs[0];
  const unsigned char* ubase = s.p[1] + (int64_t)b * s.fs[1];
  const unsigned char* vbase = SF::PLANAR ? s.p[2] + (int64_t)b * s.fs[2] : ubase;
  const int64_t pitch = s.pitch[0], upitch = s.pitch[1], vpitch = SF::PLANAR ? s.pitch[2] : s.pitch[1];
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
  const int xa = x_lo & ~(ALIGN - 1);                    // LDS column 0 <-> frame column xa
  const int ww = min(x_hi + n_ - xa, INW);               // (<= INW: rs_pick with a margin of ALIGN)
  const int npc = SF::PSUB ? ((ww + 2 * CW - 1) / (2 * CW)) * 2 : (ww + CW - 1) / CW;       // (shared chroma pieces: tid and pi have the same parity)
  int y_lo, y_hi;
  tap_range(oy0, H, oh, antialias, y_lo, n_);
  tap_range(oy_end - 1, H, oh, antialias, y_hi, n_);
  const int y_end = y_hi + n_;
  const Taps tx = make_taps(ox, W, ow, antialias);
  float wxs[MT];
#pragma unroll
  for (int jx = 0; jx < MT; ++jx) wxs[jx] = jx < tx.n ? tap_w(tx, jx) : 0.f;
  const int xoff = tx.lo - xa;

  const bool loader = tid < 4 * npc;
  const int ri = tid / npc, pi = tid - ri * npc;          // row pair of the group, piece
  const bool odd = (tid & 1) != 0;
  typename SF::SChunk pv;
  auto load_group = [&](const int r0) __attribute__((always_inline)) {
    const int row = r0 + 2 * ri;
    pv.zero();
    if (loader && row < y_end) pv.load(base, pitch, ubase, upitch, vbase, vpitch, row, xa + CW * pi, H, W, odd);     // (reads no row >= H)
  };
  int oy_next = oy0 + part;
  const int ye0 = y_lo & ~1;
  load_group(ye0);
  for (int r0 = ye0; r0 < y_end; r0 += RS_GI) {
    if (loader) {       // whole pieces, four pixels per LDS store (columns past ww and rows past y_end receive values nobody reads)
      uint4 cu[SF::NCR], cv[SF::NCR];
#pragma unroll
      for (int h = 0; h < SF::NCR; ++h) pv.chroma(h, odd, cu[h], cv[h]);
#pragma unroll
      for (int k4 = 0; k4 < CW / 4; ++k4) {
        float px[2][3][4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int q = 4 * k4 + e;
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            float rgb[3];
            SF::rgb(dec, pv.lum(h, q), SF::SChunk::cb(cu[h % SF::NCR], q), SF::SChunk::cr(cv[h % SF::NCR], q), rgb);
#pragma unroll
            for (int c = 0; c < 3; ++c) px[h][c][e] = rgb[c];
          }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int c = 0; c < 3; ++c)
            *reinterpret_cast<f32x4*>(In + ((2 * ri + h) * 3 + c) * INW + CW * pi + 4 * k4) = f32x4{px[h][c][0], px[h][c][1], px[h][c][2], px[h][c][3]};
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

// Tile form of the tail: embed_tail_kernel (shell.hip) on YUV frames (described for 4:2:0; SY = 0 below).  Workgroup = 256 columns x 16 rows of one frame (a tile starts on an
// even row: a chroma row belongs to one tile).  The tile's samples + a 2-pixel halo (20 luma rows of NVW columns from x0 - SPP, 10 chroma
// rows) are staged in LDS once as stored words, piece by piece; luminance and blend both read the pixel from there.  The arithmetic between
// decode and encode is embed_tail_kernel's (43-tap JND, the same taps, key-frame expansion and blend); a thread owns one column and walks the
// rows in pairs, the horizontal half of the 2 x 2 chroma sum comes from the neighbouring lane.  The watermarked tile is collected in LDS as
// output words and leaves as 16-byte pieces (16 luma rows, 8 chroma rows of 256 samples: pairs, or U then V).
// With SY = 0 the window holds a chroma row per luma row (20) and the tile leaves 16 chroma rows; 4:4:4 rows hold 2 x NVW / 2 x 256 samples.
// LDS: 55 - 69 KB for 4:2:0, up to 98 KB for yuv444p10 (one workgroup per CU): this form serves frames too small for the row-streaming one.
constexpr int NVR = TTH + 2 * HALO;
// GEO: YuvGeo (grid form) or YuvClipsGeo (list form: F, H, W, total_key and the first frames of delta / hmap_lowres are the slot's).
template <class SF, class GEO = YuvGeo>
__global__ __launch_bounds__(256) void embed_tail_yuv_kernel(TailArgs a, JndTaps k, GEO geo) {
  using S = typename SF::S;
  constexpr int SPP = SF::SPP, NVW = SF::NVW, NPY = SF::NPY, NPC = SF::NPC, CRS = SF::CRS, PPR = SF::PPR, OCW = SF::OCW, OPC = SF::OPC;
  constexpr int SY = SF::SY, NVC = NVR >> SY, NOC = TTH >> SY;       // chroma rows of the window, of the output tile
  __shared__ __attribute__((aligned(16))) S YS[NVR * NVW];
  __shared__ __attribute__((aligned(16))) S CS[NVC * CRS];
  __shared__ __attribute__((aligned(16))) S Yo[TTH * TTW];
  __shared__ __attribute__((aligned(16))) S Co[NOC * OCW];
  __shared__ float L[TLW * NVR];
  __shared__ float Dw[3 * DW_W * DW_H];
  __shared__ int ty_lo[TTH], ty_n[TTH];
  __shared__ float ty_w[TTH][4];
  __shared__ int s_xhi, s_nmax, s_xlo;
  const YuvAt at = yuv_at(geo);
  yuv_tail_args(geo, at.k, a);
  const auto& g = yuv_geo(geo, at.k);
  const int x0 = at.bx * TTW, y0 = at.by * TTH, f = at.f;
  const bool full_jnd = a.attenuate && !a.hmap_lowres;
  if (threadIdx.x == 0) { s_xhi = 0; s_nmax = 0; }
  {     // frame samples -> LDS: NVR x NPY luma pieces, then NVC x NPC chroma pieces; all loads of a thread issued before its stores
    constexpr int NTY = NVR * NPY, NTASK = NTY + NVC * NPC, NIT = (NTASK + 255) / 256;
    uint4 v[NIT];
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int t = threadIdx.x + 256 * i;
      v[i] = uint4{0u, 0u, 0u, 0u};
      if (t < NTY) {
        const int r = t / NPY, p = t - r * NPY;
        const int gy = y0 - HALO + r;
        const bool need = full_jnd || (r >= HALO && r < HALO + TTH);
        if (need && gy >= 0 && gy < a.H) v[i] = SF::ld16(g.s.p[0] + (int64_t)f * g.s.fs[0] + (int64_t)gy * g.s.pitch[0], x0 - SPP + SPP * p, a.W);
      } else if (t < NTASK) {
        const int r = (t - NTY) / NPC, p = (t - NTY) - r * NPC;
        const int gy = ((y0 - HALO) >> SY) + r;
        const bool need = full_jnd || (r >= (HALO >> SY) && r < ((HALO + TTH) >> SY));
        int pl, col, cw;
        SF::cpiece(p, x0, a.W, pl, col, cw);
        if (need && gy >= 0 && gy < SF::crows(a.H)) v[i] = SF::ld16(g.s.p[pl] + (int64_t)f * g.s.fs[pl] + (int64_t)gy * g.s.pitch[pl], col, cw);
      }
    }
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int t = threadIdx.x + 256 * i;
      if (t < NTY) *reinterpret_cast<uint4*>(reinterpret_cast<unsigned char*>(YS) + 16 * t) = v[i];
      else if (t < NTASK) *reinterpret_cast<uint4*>(reinterpret_cast<unsigned char*>(CS) + 16 * (t - NTY)) = v[i];
    }
  }
  __syncthreads();
  // decoded, clamped pixel at tile row rr (0 .. NVR - 1 <-> frame row y0 - 2 + rr) and window column wc (<-> frame column x0 - SPP + wc)
  auto pixel = [&](const int rr, const int wc, float (&rgb)[3]) __attribute__((always_inline)) {
    float cb, cr;
    SF::lchroma(CS + (rr >> SY) * CRS, wc, cb, cr);
    SF::rgb(g.dec, SF::val(YS[rr * NVW + wc]), cb, cr, rgb);
  };
  if (full_jnd) {       // luminance of the tile + halo, zero outside the frame (conv zero padding)
    auto lum_column = [&](const int lxx) __attribute__((always_inline)) {
      const int gx = x0 + lxx - HALO;
#pragma unroll 4
      for (int rr = 0; rr < NVR; ++rr) {
        const int gy = y0 + rr - HALO;
        float v = 0.f;
        if (gx >= 0 && gx < a.W && gy >= 0 && gy < a.H) {
          float rgb[3];
          pixel(rr, lxx + SPP - HALO, rgb);
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

  const int lasty = min(TTH, a.H - y0) - 1;              // odd where H is even (SY = 1); with an odd H the last row has no partner
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
  for (int ly0 = 0; ly0 <= lasty; ly0 += 2) {             // every lane runs every pair: the chroma sum crosses lanes
    float cbs = 0.f, crs = 0.f;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int ly = ly0 + q;
      const int y = y0 + ly;
      const bool live = xin && (SY || ly <= lasty);
      if (live) {
        float px[3];
        pixel(ly + HALO, lx + SPP, px);
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
        Yo[ly * TTW + lx] = SF::word(SF::aff(g.enc, 0, v[0], v[1], v[2]));
        cbs += SF::aff(g.enc, 1, v[0], v[1], v[2]);
        crs += SF::aff(g.enc, 2, v[0], v[1], v[2]);
      }
      if (!SY || q == 1) {                                // the block's rows are complete
        SF::ochroma(Co + (ly >> SY) * OCW, lx, live, cbs, crs);
        cbs = 0.f; crs = 0.f;
      }
    }
  }
  __syncthreads();      // Yo, Co
  for (int t = threadIdx.x; t < TTH * PPR; t += 256) {
    const int r = t / PPR, pc = t - r * PPR;
    const int col = x0 + SPP * pc;
    if (y0 + r < a.H && col < a.W)
      SF::st16(const_cast<unsigned char*>(g.d.p[0]) + (int64_t)f * g.d.fs[0] + (int64_t)(y0 + r) * g.d.pitch[0], col, a.W, Yo + SPP * t);
  }
  for (int t = threadIdx.x; t < NOC * OPC; t += 256) {
    const int r = t / OPC, pc = t - r * OPC;
    int pl, col, cw;
    SF::opiece(pc, x0, a.W, pl, col, cw);
    if ((y0 >> SY) + r < SF::crows(a.H) && col < cw)
      SF::st16(const_cast<unsigned char*>(g.d.p[pl]) + (int64_t)f * g.d.fs[pl] + (int64_t)((y0 >> SY) + r) * g.d.pitch[pl], col, cw, Co + SPP * t);
  }
}

// Row-streaming form of the tail: embed_tail_stream_kernel's structure (shell.hip: 256 columns x a strip of rows walked in groups of SG = 4,
// luminance ring, accumulators of the separable JND stencils, double-buffered watermark window, ONE barrier per group) with the frame's words
// staged through LDS as 16-byte pieces.  A group's 4 luma rows (NPY pieces each) and 2 chroma rows (NPC pieces each) are <= 208 loads, one per
// thread, requested two groups ahead of their use: loaded during group it - 1, written to the word stage before the barrier of group it, read
// by every thread (own column, halo columns) at the top of group it + 1.  Strips start on a multiple of four rows, so the two row pairs of a
// group are whole 2 x 2 blocks: the horizontal half of the chroma sum comes from the neighbouring lane.  The group's words (4 x 256 luma,
// 2 x 256 chroma) are collected in LDS and leave after the next barrier as <= 192 pieces, one per thread.
// SY = 0 (4:2:2, 4:4:4): a group carries FOUR chroma rows, reduced row by row (a lane-pair mean, or none).  The 8-bit surfaces still move
// one piece per thread each way (<= 216 in, <= 192 out); the 16-bit ones have 272 - 408 pieces in and 256 - 384 out, so a thread holds up to
// two (NLT, NOT).  4:4:4 doubles the chroma pieces per row, not the tile: 256 columns stay.  Static LDS grows from 7 - 13 KB (4:2:0) to 9 - 26 KB;
// with the dynamic part (12 KB luminance ring + 13 KB (Cd = 1) or 39 KB (Cd = 3) watermark windows) the worst case, yuv444p10 with the
// full-resolution heat-map and Cd = 3, is 78 KB: two workgroups per CU of 160 KB, as for yuv420p10 (65 KB); its 144 VGPRs allow three waves
// per SIMD, so LDS and registers bind at the same two to three workgroups.
template <class SF, bool JND, int CD>
__global__ __launch_bounds__(256) void embed_tail_yuv_stream_kernel(TailArgs a, JndTaps k, YuvGeo g, const int strip) {
  using S = typename SF::S;
  constexpr int SPP = SF::SPP, NSW = SF::NVW, NPY = SF::NPY, NPC = SF::NPC, CRS = SF::CRS, PPR = SF::PPR, OCW = SF::OCW, OPC = SF::OPC;
  constexpr int SY = SF::SY, NCG = SG >> SY;                   // chroma rows of a group
  constexpr int NLD = SG * NPY + NCG * NPC, NST = SG * PPR + NCG * OPC;
  constexpr int NLT = (NLD + 255) / 256, NOT = (NST + 255) / 256;               // pieces per thread and group, in and out: 1 for every 4:2:0 surface
  static_assert(NLT <= 2 && NOT <= 2, "at most two pieces per thread and group");
  extern __shared__ float dyn_smem[];
  float* Lr = dyn_smem;                                        // [RING][TLW] luminance ring (JND only)
  float* DwB = dyn_smem + (JND ? RING * TLW : 0);              // [2][Cd][DW_H][DW_W] watermark source windows
  __shared__ __attribute__((aligned(16))) S Bst[2][SG * NSW + NCG * CRS];          // incoming words: rows 0-3 luma, then the group's chroma rows
  __shared__ __attribute__((aligned(16))) S Ost[2][SG * TTW + NCG * OCW];          // outgoing words, same row order
  __shared__ int ty_lo[2][SUBR], ty_n[2][SUBR], s_wy0[2];
  __shared__ float ty_w[2][SUBR][4];
  __shared__ int s_xhi, s_xlo;
  constexpr int dwsz = CD * DW_W * DW_H;
  const int x0 = blockIdx.x * TTW, y0 = blockIdx.y * strip, f = blockIdx.z;
  const int ys_end = min(a.H, y0 + strip);
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

  // one 16-byte piece per loader thread and group: group gi brings rows y0 + 4 gi + 2 .. + 5 and the two chroma rows under them
  // (task lx + 256 i, i < NLT: the 16-bit 4:2:2 and 4:4:4 surfaces have 272 - 408 pieces per group)
  bool ldr[NLT], lluma[NLT];
  int lrow[NLT], lcol[NLT], lcw[NLT];
  const unsigned char* lbase[NLT];
  int64_t lpitch[NLT];
#pragma unroll
  for (int i = 0; i < NLT; ++i) {
    const int t = lx + 256 * i;
    ldr[i] = t < NLD;
    lluma[i] = t < SG * NPY;
    lrow[i] = lluma[i] ? t / NPY : (t - SG * NPY) / NPC;
    const int lpc = lluma[i] ? t - lrow[i] * NPY : (t - SG * NPY) - lrow[i] * NPC;
    int lpl = 0;
    lcol[i] = x0 - SPP + SPP * lpc;
    lcw[i] = a.W;
    if (!lluma[i]) SF::cpiece(lpc, x0, a.W, lpl, lcol[i], lcw[i]);
    lbase[i] = g.s.p[lpl] + (int64_t)f * g.s.fs[lpl];
    lpitch[i] = g.s.pitch[lpl];
  }
  struct Pieces { uint4 v[NLT]; };
  auto load_piece = [&](const int gi) __attribute__((always_inline)) -> Pieces {
    const int r0 = y0 + SG * gi + HALO;                        // even
    Pieces pc;
#pragma unroll
    for (int i = 0; i < NLT; ++i) {
      pc.v[i] = uint4{0u, 0u, 0u, 0u};
      if (ldr[i]) {
        const int gy = lluma[i] ? r0 + lrow[i] : (r0 >> SY) + lrow[i];
        const int lim = lluma[i] ? a.H : SF::crows(a.H);
        if (gy >= 0 && gy < lim) pc.v[i] = SF::ld16(lbase[i] + (int64_t)gy * lpitch[i], lcol[i], lcw[i]);
      }
    }
    return pc;
  };
  auto stash = [&](const int slot, const Pieces& pc) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NLT; ++i)
      if (ldr[i]) *reinterpret_cast<uint4*>(reinterpret_cast<unsigned char*>(Bst[slot]) + 16 * (lx + 256 * i)) = pc.v[i];
  };
  auto pixel = [&](const int slot, const int q, const int wc, float (&rgb)[3]) __attribute__((always_inline)) {
    const S* B = Bst[slot];
    float cb, cr;
    SF::lchroma(B + SG * NSW + (q >> SY) * CRS, wc, cb, cr);
    SF::rgb(g.dec, SF::val(B[q * NSW + wc]), cb, cr, rgb);
  };
  Pieces pv = load_piece(-1);
  stash(0, pv);

  const KeyMix km = key_mix(a, f, CD);                   // value = wa*key[ka] + wb*key[kb]
  const float wa = km.wa, wb = km.wb;
  const float *dka = km.dka, *dkb = km.dkb, *hml = km.hml;
  const int splane = a.Sh * a.Sw;
  __syncthreads();                                             // s_xlo / s_xhi, word stage of group -1
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
        const bool luma = t < SG * PPR;
        const int orow = luma ? t / PPR : (t - SG * PPR) / OPC, pc = luma ? t - orow * PPR : (t - SG * PPR) - orow * OPC;
        const int yb = y0 + SG * gi;
        const int y = luma ? yb + orow : yb + (orow << SY);                       // (the first luma row of a chroma row's block)
        int pl = 0, col = x0 + SPP * pc, cw = a.W;
        if (!luma) SF::opiece(pc, x0, a.W, pl, col, cw);
        if (y < ys_end && col < cw)
          SF::st16(const_cast<unsigned char*>(g.d.p[pl]) + (int64_t)f * g.d.fs[pl] + (int64_t)(luma ? y : (y >> SY)) * g.d.pitch[pl], col, cw,
                   Ost[gi & 1] + SPP * t);
      }
    }
  };

  const int nrows = ys_end - y0;
  const int niter = (nrows + SG - 1) / SG;
  float acc_la[2 * SG], acc_gx[2 * SG], acc_gy[2 * SG];
#pragma unroll
  for (int i = 0; i < 2 * SG; ++i) { acc_la[i] = 0.f; acc_gx[i] = 0.f; acc_gy[i] = 0.f; }
  float hist[2][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
  pv = load_piece(0);
  stage(0, 0);
  for (int it = -1; it < niter; ++it) {
    const int r0 = y0 + SG * it + HALO;                       // first incoming row of this group; its output rows are r0 - 2 .. r0 + 1
    const int slot0 = ((it + 1) % 3) * SG;
    const int bs = (it + 1) & 1;
    float cu[SG][3];
#pragma unroll
    for (int q = 0; q < SG; ++q) pixel(bs, q, lx + SPP, cu[q]);
    if (JND) {
#pragma unroll
      for (int q = 0; q < SG; ++q) {
        const int gy = r0 + q;
        const bool rok = gy >= 0 && gy < a.H;
        Lr[(slot0 + q) * TLW + lx + HALO] = (rok && xin) ? lum255(cu[q][0], cu[q][1], cu[q][2]) : 0.f;
        if (hal) {
          float hp[3];
          pixel(bs, q, hl + SPP - HALO, hp);
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
    S* Og = Ost[it & 1];
    float cbs = 0.f, crs = 0.f;
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
      const bool live = it >= 0 && y < ys_end && xin;
      if (live) {
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
        Og[j * TTW + lx] = SF::word(SF::aff(g.enc, 0, v[0], v[1], v[2]));
        cbs += SF::aff(g.enc, 1, v[0], v[1], v[2]);
        crs += SF::aff(g.enc, 2, v[0], v[1], v[2]);
      }
      if (!SY || (j & 1)) {                                    // the block's rows are complete: every lane takes part in the exchange
        SF::ochroma(Og + SG * TTW + (j >> SY) * OCW, lx, live, cbs, crs);
        cbs = 0.f; crs = 0.f;
      }
    }
#pragma unroll
    for (int i = 0; i < SG; ++i) {
      acc_la[i] = acc_la[i + SG]; acc_gx[i] = acc_gx[i + SG]; acc_gy[i] = acc_gy[i + SG];
      acc_la[i + SG] = 0.f; acc_gx[i + SG] = 0.f; acc_gy[i + SG] = 0.f;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) { hist[0][c] = cu[2][c]; hist[1][c] = cu[3][c]; }
  }
  __syncthreads();
  store_group(niter - 1);
}

// ---- host side, shared by the entry points of yuv420.hip and yuv4xx.hip (SURFACE: vs_yuv420_surface_t or vs_yuv_surface_t, DESC: their tail descriptors)

// the layout of a surface's samples: 0 interleaved 8-bit (nv12, nv16), 1 planar 8-bit (i420, yuv422p, yuv444p), 2 interleaved 10-bit in the
// high bits (p010, p210), 3 planar 10-bit in the low bits (yuv420p10, yuv422p10, yuv444p10); -1: no such layout
template <class SURFACE>
int surface_format(const SURFACE& s) {
  if (s.depth == 8 && !s.msb_aligned) return s.planar ? 1 : 0;
  if (s.depth == 10 && !s.planar && s.msb_aligned == 1) return 2;
  if (s.depth == 10 && s.planar == 1 && !s.msb_aligned) return 3;
  return -1;
}
// planes present, every pitch holds a row, frames of a plane do not overlap  (sx, sy: the chroma shifts)
template <class SURFACE>
bool surface_ok(const SURFACE& s, int sx, int sy, int F, int H, int W) {
  const int np = s.planar ? 3 : 2, bps = s.depth > 8 ? 2 : 1;
  for (int i = 0; i < np; ++i) {
    const int64_t rowb = (int64_t)(i == 0 || !s.planar ? W : W >> sx) * bps, rows = i == 0 ? H : H >> sy;
    if (!s.plane[i] || s.pitch[i] < rowb) return false;
    if (F > 1 && s.frame_stride[i] < s.pitch[i] * (rows - 1) + rowb) return false;
  }
  return true;
}
template <class SURFACE>
YuvSurf dev_surface(const SURFACE& s) {
  YuvSurf d{};
  for (int i = 0; i < 3; ++i) {
    d.p[i] = static_cast<const unsigned char*>(s.plane[i]);
    d.pitch[i] = s.pitch[i];
    d.fs[i] = s.frame_stride[i];
  }
  return d;
}

// the kernels of one surface trait, for launch_resize / launch_tail (shell_common.h)
template <class SF>
struct YuvKernels {
  static constexpr int ALIGN = yuv_rs_align<SF>();
  template <int OW> static auto resize_stream() { return resize_pre_yuv_stream_kernel<SF, OW>; }
  static auto resize_tile() { return resize_pre_yuv_kernel<SF>; }
  template <bool JND, int CD> static auto tail_stream() { return embed_tail_yuv_stream_kernel<SF, JND, CD>; }
  static auto tail_tile() { return embed_tail_yuv_kernel<SF>; }
};

// the arguments of a resize launch after the checks every entry point applies, in the order vs_resize_pre_yuv420 has always applied them
struct ResizeCall { YuvSurf s; Nv12Mat dec; int B, H, W, oh, ow, antialias; ResizeOut o; hipStream_t st; int fmt; };
template <class SURFACE>
int prep_resize(const SURFACE* src, int sx, int sy, int B, int H, int W, const float* yuv2rgb12, int oh, int ow, int antialias, float* dst_rgb,
                float mul, float add, float* dst_y, int y_step, const float* ymat3, void* stream, ResizeCall& c) {
  VS_REQUIRE(src && yuv2rgb12 && B > 0 && H > 0 && W > 0 && oh > 0 && ow > 0 && (dst_rgb || dst_y));
  VS_REQUIRE(!(H & ((1 << sy) - 1)) && !(W & ((1 << sx) - 1)));
  VS_REQUIRE(!dst_y || y_step >= 1);
  const int fmt = surface_format(*src);
  if (fmt < 0) return VS_ERR_UNSUPPORTED;
  VS_REQUIRE(surface_ok(*src, sx, sy, B, H, W));
  c = ResizeCall{dev_surface(*src), {}, B, H, W, oh, ow, antialias, resize_out(dst_rgb, mul, add, dst_y, y_step, ymat3), (hipStream_t)stream, fmt};
  for (int i = 0; i < 12; ++i) c.dec.m[i] = yuv2rgb12[i];
  return VS_OK;
}

// ... and of a tail launch (vs_embed_tail_yuv420's checks in its order)
struct TailCall { TailForm t; YuvGeo g; hipStream_t st; int fmt; };
template <class DESC>
int prep_tail(const DESC* d, int sx, int sy, void* stream, TailCall& c) {
  VS_REQUIRE(d && d->delta && d->F > 0 && d->H > 0 && d->W > 0 && d->S_h > 0 && d->S_w > 0);
  if (const int rc = tail_desc_numbers(d); rc != VS_OK) return rc;
  VS_REQUIRE(!(d->H & ((1 << sy) - 1)) && !(d->W & ((1 << sx) - 1)) && d->clamp);        // codes are only defined for values in [0, 1]
  const int fmt = surface_format(d->src);
  if (fmt < 0 || surface_format(d->dst) != fmt) return VS_ERR_UNSUPPORTED;
  VS_REQUIRE(surface_ok(d->src, sx, sy, d->F, d->H, d->W) && surface_ok(d->dst, sx, sy, d->F, d->H, d->W));
  if (const int rc = tail_desc_form(d, c.t); rc != VS_OK) return rc;
  c.g = YuvGeo{dev_surface(d->src), dev_surface(d->dst), {}, {}};
  for (int i = 0; i < 12; ++i) { c.g.dec.m[i] = d->yuv2rgb12[i]; c.g.enc.m[i] = d->rgb2yuv12[i]; }
  c.st = (hipStream_t)stream;
  c.fmt = fmt;
  return VS_OK;
}

template <class SF>
int run_resize(const ResizeCall& c) { return launch_resize<YuvKernels<SF>>(c.B, c.H, c.W, c.oh, c.ow, c.antialias, c.o, c.st, c.s, c.dec); }
template <class SF>
int run_tail(const TailCall& c) { return launch_tail<YuvKernels<SF>>(c.t.a, c.t.k, c.g, c.t.stream_form, c.t.full_jnd, c.st); }

}  // namespace
