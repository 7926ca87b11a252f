// Model-level entry points of the C-ABI (last row): an opaque vs_model_t built from a card + the reference
// state_dict (HOST fp32 tensors by name), immutable after creation, and whole-path calls at the granularity of
// Wam.embed / Videoseal.embed (wam.py:134-204, videoseal.py:258-350) and detect (wam.py:206-234, videoseal.py:352-388).
// Everything here is host code: weight preparation (eval-BatchNorm folding, [N][tap][CinP] packing, the 3 x bf16 split and the
// LDS-image blocking of engine.py) and the launch sequences of engine.py::embedder_forward / extractor_forward, issued on the
// caller's stream into the caller's workspace through the operator-level entry points of this same library.
// No allocation after vs_model_create, no synchronisation, no torch.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "vs_common.h"
#include "videoseal_half.h"

#pragma clang fp contract(off)      // host-side weight folding must round like the torch ops it restates (no fused multiply-add)

namespace {

inline int rup(int v, int m) { return (v + m - 1) / m * m; }

struct HostT { const float* p; int64_t n; };

struct CW {                      // one conv / linear layer on the device
  float* wt = nullptr; float* bias = nullptr; void* split = nullptr; void* blk = nullptr;
  int N = 0, KH = 0, KW = 0, CinP = 0;
  float w_mul = 1.f;             // power of two the weights were multiplied with before the 2 x f16 split (arith 2)
};
struct RB { CW c0, c1, res; int cout = 0; };
struct Up { CW conv; CW gemm; bool lowres = false; float* lnw = nullptr; float* lnb = nullptr; RB rb; };   // gemm: nine taps at the low resolution (vs_upconv_gather_ln)
struct Down { float* lnw = nullptr; float* lnb = nullptr; CW conv, gemm; };      // gemm: the same weights as a 1x1 GEMM on the patch matrix (vs_layernorm_patch2x2)
struct Blk {
  float *wdw = nullptr, *bdw = nullptr, *lnw = nullptr, *lnb = nullptr, *gamma = nullptr, *beta = nullptr; CW pw1, pw2;
  void* fuse = nullptr; float fm1 = 1.f, fm2 = 1.f;      // weight image of the fused block kernel (vs_cnx_block) and its two power-of-two scales
};

struct Act { float* p; int B, H, W, C, ld; int64_t rows() const { return (int64_t)B * H * W; } };

}  // namespace

struct vs_model {
  vs_model_cfg_t c;
  std::vector<void*> dev;
  std::vector<int> zc;
  int bott = 0;
  // embedder
  RB inc;
  std::vector<CW> down_conv;
  std::vector<RB> down_rb, bottleneck;
  CW b0_lat, b0_msg;             // first bottleneck block with the message channels as a border-class table (engine.py::resblock_msg0)
  bool b0_table = false;
  // engine.py::_msg_vectors_pack: the pointwise consumers of the message channels take them as one vector per message -- b0_msg carries the
  // rows of res_conv's message columns (+ res_conv.bias) at msgv_off_res and of the first Upsample GEMM's message-skip columns (x connect_scale)
  // at msgv_off_up; b0_res_lat / up0_xl are those layers without the message columns
  CW b0_res_lat, up0_xl;
  bool msgv = false;
  int msgv_off_res = 0, msgv_off_up = 0;
  std::vector<Up> ups;
  float *outc_w = nullptr, *outc_b = nullptr, *table = nullptr;
  // extractor
  CW stem, head, head_gemm;      // head_gemm: the same 3x3 weights seen as a 1x1 GEMM on the patch matrix (vs_im2col3x3)
  float *stem_lnw = nullptr, *stem_lnb = nullptr, *head_lnw = nullptr, *head_lnb = nullptr, *lin_w = nullptr, *lin_b = nullptr;
  Down down[3];
  std::vector<Blk> stages[4];
  float ymat[3];
  float taps43[43];
  float yuv2rgb12[12], rgb2yuv12[12];      // NV12 colour affines (io_u8 = 2): BT.709 limited range until vs_model_set_nv12_color
  int arith = 3;                 // arithmetic of the split planes (vs_conv_desc_t::arith)
  bool ok = true;
};

static constexpr float A_MUL = 16.f;      // engine.py::A_MUL
static constexpr float A_MUL_GRN = 1.f;   // engine.py::A_MUL_GRN (the GRN-scaled operand of pwconv2)

namespace {

int xld(int C) { return C >= 128 ? rup(C, 32) : rup(C, 4); }     // engine.py::_xld

// ---------------------------------------------------------------- weight preparation (host) + upload
struct Packer {
  vs_model* m;
  const std::map<std::string, HostT>& sd;
  bool fail = false;

  const HostT& get(const std::string& k, bool optional = false) {
    static HostT none{nullptr, 0};
    auto it = sd.find(k);
    if (it == sd.end()) { if (!optional) fail = true; return none; }
    return it->second;
  }
  template <typename T>
  T* upload(const std::vector<T>& v) {
    void* d = nullptr;
    if (v.empty()) return nullptr;
    if (hipMalloc(&d, v.size() * sizeof(T)) != hipSuccess) { fail = true; return nullptr; }
    if (hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) fail = true;
    m->dev.push_back(d);
    return static_cast<T*>(d);
  }
  float* vec(const std::string& k, int padded = 0) {
    const HostT& t = get(k);
    if (!t.p) return nullptr;
    std::vector<float> v((size_t)std::max<int64_t>(t.n, padded), 0.f);
    std::copy(t.p, t.p + t.n, v.begin());
    return upload(v);
  }
  // fp32 -> three bf16 terms by truncation (engine.py::split_bf16x3); planes [3][N][K]
  static void split3(const std::vector<float>& w, std::vector<uint16_t>& planes) {
    const size_t n = w.size();
    planes.assign(3 * n, 0);
    for (size_t i = 0; i < n; ++i) {
      float r = w[i];
      for (int p = 0; p < 3; ++p) {
        uint32_t u;
        std::memcpy(&u, &r, 4);
        const uint32_t hi = u & 0xffff0000u;
        planes[p * n + i] = (uint16_t)(hi >> 16);
        float h;
        std::memcpy(&h, &hi, 4);
        r = r - h;
      }
    }
  }
  // engine.py::split_f16x2: w * w_mul = hi + lo in round-to-nearest f16, w_mul = the power of two that puts max|w| into [2^13, 2^14)
  static float split2(const std::vector<float>& w, std::vector<uint16_t>& planes) {
    const size_t n = w.size();
    planes.assign(2 * n, 0);
    float amax = 0.f;
    for (float v : w) amax = std::max(amax, std::fabs(v));
    int kw = 0;
    if (amax > 0.f && std::isfinite(amax)) { int e; (void)std::frexp(amax, &e); kw = std::max(-100, std::min(100, 14 - e)); }
    for (size_t i = 0; i < n; ++i) {
      const float ws = std::ldexp(w[i], kw);
      const _Float16 hi = (_Float16)ws;
      const _Float16 lo = (_Float16)(ws - (float)hi);
      std::memcpy(&planes[i], &hi, 2);
      std::memcpy(&planes[n + i], &lo, 2);
    }
    return std::ldexp(1.f, kw);
  }
  // engine.py::pack_blocked: [P][N][K] -> [ceil(N/32)][K/16][P][64 slots][8], chunk order (channel chunk, tap), bank swizzle
  static void blocked(const std::vector<uint16_t>& planes, int n, int k, int ntaps, std::vector<uint16_t>& out) {
    const int NPL = (int)(planes.size() / ((size_t)n * k));
    const int G = (n + 31) / 32, nch = k / 16, spt = nch / ntaps;
    out.assign((size_t)G * nch * NPL * 64 * 8, 0);
    for (int p = 0; p < NPL; ++p)
      for (int row = 0; row < n; ++row) {
        const int g = row / 32, r = row % 32;
        for (int tap = 0; tap < ntaps; ++tap)
          for (int cc = 0; cc < spt; ++cc) {
            const int blkidx = cc * ntaps + tap;                  // step order of the kernels
            for (int h = 0; h < 2; ++h) {
              const int slot = 2 * r + (h ^ ((r >> 3) & 1));
              const uint16_t* src = &planes[(size_t)p * n * k + (size_t)row * k + (size_t)(tap * spt + cc) * 16 + h * 8];
              uint16_t* dst = &out[((((size_t)g * nch + blkidx) * NPL + p) * 64 + slot) * 8];
              std::copy(src, src + 8, dst);
            }
          }
      }
  }
  // engine.py::pack_cnx_block: weight image of csrc/convnext_fused.hip for one ConvNeXt block.  w1 [4C][C], w2 [C][4C], b1 / beta [4C].
  // Per block of 32 h-channels: W1 rows as A fragments [k-step][plane][half][row 32][8]; W2 as B fragments [n-block][s][plane][half][n 32][8]
  // with the reduction index enumerated as k(s, half, v) = 8 (2 s + v / 4) + 4 half + v % 4; then 256 floats: b1[32], beta[32], zeros.
  void* cnx_image(const HostT& w1, const HostT& b1, const HostT& w2, const HostT& beta, int C, float& m1, float& m2) {
    const int H4 = 4 * C, nhb = H4 / 32, ks1 = C / 16, nb = C / 32;
    if (!w1.p || !b1.p || !w2.p || !beta.p || w1.n != (int64_t)H4 * C || w2.n != (int64_t)H4 * C || b1.n < H4 || beta.n < H4) return nullptr;
    std::vector<uint16_t> p1, p2;
    m1 = split2(std::vector<float>(w1.p, w1.p + w1.n), p1);          // [plane][4C][C]
    m2 = split2(std::vector<float>(w2.p, w2.p + w2.n), p2);          // [plane][C][4C]
    const size_t per_hb = (size_t)2048 * ks1 + (size_t)4096 * nb + 1024;      // W1 fragments, W2 fragments (two k-steps per n-block), 256 floats
    if ((int64_t)(per_hb * nhb) != vs_cnx_block_image_bytes(C)) { fail = true; return nullptr; }      // (layout drifted from convnext_fused.hip: loud)
    std::vector<uint8_t> img(per_hb * nhb, 0);
    const size_t n1 = (size_t)H4 * C;
    for (int hb = 0; hb < nhb; ++hb) {
      uint16_t* i1 = reinterpret_cast<uint16_t*>(img.data() + per_hb * hb);
      uint16_t* i2 = i1 + (size_t)1024 * ks1;
      float* aux = reinterpret_cast<float*>(img.data() + per_hb * hb + (size_t)2048 * ks1 + (size_t)4096 * nb);
      for (int ks = 0; ks < ks1; ++ks)
        for (int pl = 0; pl < 2; ++pl)
          for (int half = 0; half < 2; ++half)
            for (int mm = 0; mm < 32; ++mm)
              for (int v = 0; v < 8; ++v)
                i1[((((size_t)ks * 2 + pl) * 2 + half) * 32 + mm) * 8 + v] = p1[pl * n1 + (size_t)(hb * 32 + mm) * C + ks * 16 + half * 8 + v];
      for (int b = 0; b < nb; ++b)
        for (int s2 = 0; s2 < 2; ++s2)
          for (int pl = 0; pl < 2; ++pl)
            for (int half = 0; half < 2; ++half)
              for (int n = 0; n < 32; ++n)
                for (int vh = 0; vh < 2; ++vh)
                  for (int e = 0; e < 4; ++e)
                    i2[((((((size_t)b * 2 + s2) * 2 + pl) * 2 + half) * 32 + n) * 2 + vh) * 4 + e] =
                        p2[pl * n1 + (size_t)(b * 32 + n) * H4 + 32 * hb + 8 * (2 * s2 + vh) + 4 * half + e];
      for (int i = 0; i < 32; ++i) { aux[i] = b1.p[hb * 32 + i]; aux[32 + i] = beta.p[hb * 32 + i]; }
    }
    return upload(img);
  }
  void finish(CW& cw, const std::vector<float>& wt, const std::vector<float>& bias, bool has_bias, CW* as_gemm = nullptr) {
    cw.wt = upload(wt);
    if (has_bias) cw.bias = upload(bias);
    std::vector<uint16_t> planes, blk;
    if (m->arith == 2) cw.w_mul = split2(wt, planes);
    else split3(wt, planes);
    cw.split = upload(planes);
    blocked(planes, cw.N, cw.KH * cw.KW * cw.CinP, cw.KH * cw.KW, blk);
    cw.blk = upload(blk);
    if (as_gemm) {                 // same rows read as one K run of KH*KW*CinP (K order (tap, channel)): blocked image in plain K order
      *as_gemm = cw;
      as_gemm->CinP = cw.KH * cw.KW * cw.CinP;
      as_gemm->KH = as_gemm->KW = 1;
      blocked(planes, cw.N, as_gemm->CinP, 1, blk);
      as_gemm->blk = upload(blk);
    }
  }
  // engine.py::pack_conv: [N,Cin,KH,KW] -> [N][tap][CinP], optional per-row scale (folded BatchNorm)
  void conv(CW& cw, const std::string& wkey, int cin, int kh, int kw, int in_ld, const std::vector<float>* scale,
            const std::vector<float>* bias_v, const std::string& bias_key, CW* as_gemm = nullptr, std::vector<float>* keep_wt = nullptr) {
    const HostT& w = get(wkey);
    if (!w.p) return;
    const int n = (int)(w.n / ((int64_t)cin * kh * kw));
    const int cinp = rup(std::max(in_ld, cin), 16);
    cw.N = n; cw.KH = kh; cw.KW = kw; cw.CinP = cinp;
    std::vector<float> wt((size_t)n * kh * kw * cinp, 0.f);
    for (int o = 0; o < n; ++o)
      for (int c = 0; c < cin; ++c)
        for (int t = 0; t < kh * kw; ++t) {
          float v = w.p[((size_t)o * cin + c) * kh * kw + t];
          if (scale) v = v * (*scale)[o];
          wt[((size_t)o * kh * kw + t) * cinp + c] = v;
        }
    std::vector<float> b;
    bool hb = false;
    if (bias_v) { b = *bias_v; hb = true; }
    else if (!bias_key.empty()) { const HostT& t = get(bias_key); if (t.p) { b.assign(t.p, t.p + t.n); hb = true; } }
    finish(cw, wt, b, hb, as_gemm);
    if (keep_wt) *keep_wt = std::move(wt);
  }
  // engine.py::_pack_embedder (Upsample groups): [Co,Cin,3,3] -> rows (tap, channel) of a 1x1 GEMM on the low-resolution [x | skip] map
  void upconv9(CW& cw, const std::string& wkey, int cin, int cout, std::vector<float>* keep_wt = nullptr) {
    const HostT& w = get(wkey);
    if (!w.p) return;
    const int cinp = rup(cin, 16);
    cw.N = 9 * cout; cw.KH = 1; cw.KW = 1; cw.CinP = cinp;
    std::vector<float> wt((size_t)9 * cout * cinp, 0.f);
    for (int o = 0; o < cout; ++o)
      for (int c = 0; c < cin; ++c)
        for (int t = 0; t < 9; ++t) wt[((size_t)t * cout + o) * cinp + c] = w.p[((size_t)o * cin + c) * 9 + t];
    finish(cw, wt, {}, false);
    if (keep_wt) *keep_wt = std::move(wt);
  }
  // engine.py::pack_patch_conv: kw pixels of a row are one run of kw*pix_ld floats -> KH x 1 conv with Cin' = kw*pix_ld
  void patch_conv(CW& cw, const std::string& wkey, int cin, int k, int pix_ld, const std::string& bias_key, CW* as_gemm = nullptr) {
    const HostT& w = get(wkey);
    if (!w.p) return;
    const int n = (int)(w.n / ((int64_t)cin * k * k));
    const int run = k * pix_ld, cinp = rup(run, 16);
    cw.N = n; cw.KH = k; cw.KW = 1; cw.CinP = cinp;
    std::vector<float> wt((size_t)n * k * cinp, 0.f);
    for (int o = 0; o < n; ++o)
      for (int c = 0; c < cin; ++c)
        for (int ky = 0; ky < k; ++ky)
          for (int kx = 0; kx < k; ++kx) wt[((size_t)o * k + ky) * cinp + kx * pix_ld + c] = w.p[(((size_t)o * cin + c) * k + ky) * k + kx];
    const HostT& bt = get(bias_key);
    std::vector<float> b;
    if (bt.p) b.assign(bt.p, bt.p + bt.n);
    finish(cw, wt, b, bt.p != nullptr, as_gemm);
  }
  void bn_fold(const std::string& p, std::vector<float>& s, std::vector<float>& b) {          // engine.py::_bn_fold
    const HostT &w = get(p + ".weight"), &bi = get(p + ".bias"), &mu = get(p + ".running_mean"), &var = get(p + ".running_var");
    if (!w.p || !bi.p || !mu.p || !var.p) return;
    s.resize(w.n); b.resize(w.n);
    for (int64_t i = 0; i < w.n; ++i) {
      s[i] = w.p[i] / std::sqrt(var.p[i] + 1e-5f);
      b[i] = bi.p[i] - mu.p[i] * s[i];
    }
  }
  // engine.py::resblock_msg0: c0 of the first bottleneck block split into its latent columns (3x3, K = 9*nlat) and the per-tap
  // message columns (rows (tap, n), K = hidden) from the BN-folded packed weight [N][9][cinp]
  // extra / extra_bias: further rows [rows][hidden] of the message GEMM behind the 9 n tap rows (engine.py::_msg_vectors_pack)
  void msg_table_convs(CW& lat, CW& msg, const std::vector<float>& wt, const std::vector<float>& bias, int n, int cinp, int nlat, int hidden,
                       const std::vector<float>* extra = nullptr, const std::vector<float>* extra_bias = nullptr) {
    std::vector<float> wl((size_t)n * 9 * nlat), wm((size_t)9 * n * hidden);
    for (int o = 0; o < n; ++o)
      for (int t = 0; t < 9; ++t) {
        const float* src = &wt[((size_t)o * 9 + t) * cinp];
        std::copy(src, src + nlat, &wl[((size_t)o * 9 + t) * nlat]);
        std::copy(src + nlat, src + nlat + hidden, &wm[((size_t)t * n + o) * hidden]);
      }
    lat.N = n; lat.KH = 3; lat.KW = 3; lat.CinP = nlat;
    finish(lat, wl, bias, true);
    msg.N = 9 * n; msg.KH = 1; msg.KW = 1; msg.CinP = hidden;
    if (extra) {
      wm.insert(wm.end(), extra->begin(), extra->end());
      msg.N += (int)(extra->size() / hidden);
      std::vector<float> mb((size_t)9 * n, 0.f);
      mb.insert(mb.end(), extra_bias->begin(), extra_bias->end());
      finish(msg, wm, mb, true);
      return;
    }
    finish(msg, wm, {}, false);
  }
  void resblock(RB& rb, const std::string& p, int cin, std::vector<float>* keep_c0 = nullptr, std::vector<float>* keep_b0 = nullptr,
                std::vector<float>* keep_res = nullptr) {   // engine.py::_pack_resblock
    const HostT& w0 = get(p + ".double_conv.0.weight");
    if (!w0.p) return;
    const int cout = (int)(w0.n / ((int64_t)cin * 9));
    rb.cout = cout;
    std::vector<float> s0, b0, s1, b1;
    bn_fold(p + ".double_conv.1", s0, b0);
    bn_fold(p + ".double_conv.4", s1, b1);
    conv(rb.c0, p + ".double_conv.0.weight", cin, 3, 3, rup(cin, 4), &s0, &b0, "", nullptr, keep_c0);
    if (keep_b0) *keep_b0 = b0;
    conv(rb.c1, p + ".double_conv.3.weight", cout, 3, 3, rup(cout, 4), &s1, &b1, "");
    conv(rb.res, p + ".res_conv.weight", cin, 1, 1, rup(cin, 4), nullptr, nullptr, p + ".res_conv.bias", nullptr, keep_res);
  }
};

// ---------------------------------------------------------------- launch sequences
struct Runner {
  vs_model* m;
  char* ws;             // nullptr: counting pass (vs_model_workspace_bytes), no launches
  int64_t cap, used = 0;
  void* st;
  int rc = VS_OK;
  // io = 3 (vs_model_*_yuv, vs_model_*_yuv420): the surfaces and their colour affines
  const vs_yuv_surface_t* ysrc = nullptr;
  const vs_yuv_surface_t* ydst = nullptr;
  const float* ydec = nullptr;
  const float* yenc = nullptr;
  // io = 4 (vs_model_*_rgb): the packed RGB surfaces
  const vs_rgb_surface_t* psrc = nullptr;
  const vs_rgb_surface_t* pdst = nullptr;
  // io = 5 (vs_model_*_half): the half-precision surfaces
  const vs_half_surface_t* hsrc = nullptr;
  const vs_half_surface_t* hdst = nullptr;
  // vs_model_embed_psnr: the strength of every frame comes from a target PSNR (scale_out: device, [frames])
  struct Psnr { float target_db; int per_clip; float max_scale; float* scale_out; };
  const Psnr* psnr = nullptr;

  float* alloc(int64_t floats) {
    const int64_t bytes = (floats * 4 + 255) & ~(int64_t)255;
    float* p = ws ? reinterpret_cast<float*>(ws + used) : nullptr;
    used += bytes;
    if (ws && used > cap) rc = VS_ERR_BAD_ARG;
    return p;
  }
  Act act(int B, int H, int W, int C, int ld = 0) {
    if (!ld) ld = rup(C, 4);
    return Act{alloc((int64_t)B * H * W * ld), B, H, W, C, ld};
  }
  bool live() const { return ws && rc == VS_OK; }
  void chk(int code) { if (rc == VS_OK && code != VS_OK) rc = code; }

  // engine.py::conv(bias_frames= / bias2_frames=): one bias vector per frame for the NEXT conv / conv_pl call (taken and cleared by it)
  const float* fb_bias = nullptr; int64_t fb_bias_fs = 0;
  const float* fb_bias2 = nullptr; int64_t fb_bias2_fs = 0;
  void frame_bias(vs_conv_desc_t& d) {
    if (fb_bias) { d.bias = fb_bias; d.bias_fs = fb_bias_fs; }
    if (fb_bias2) { d.bias2 = fb_bias2; d.bias2_fs = fb_bias2_fs; }
    fb_bias = fb_bias2 = nullptr; fb_bias_fs = fb_bias2_fs = 0;
  }
  // engine.py::conv without the tuner: K slices, the sliced launch's tile and the GRN-finish fold as vs_conv_plan says
  void conv(const Act& x, const CW& w, const Act& out, int stride = 1, int pad = 0, int pad_mode = VS_PAD_ZERO, int act_ = VS_ACT_NONE,
            int out_coff = 0, int n_store = -1, const Act* res = nullptr, const Act* in2 = nullptr, const CW* w2 = nullptr,
            const float* a_scale = nullptr, int64_t a_scale_ld = 0, const float* a_shift = nullptr, const int* geom = nullptr,
            float* sumsq = nullptr, int cin_first = 0, bool pre_table = false, float a_mul_override = 0.f,
            const float* grn_part = nullptr, const float* grn_gamma = nullptr, int grn_hw = 0, int grn_c4 = 0, int tile_hint = 0) {
    vs_conv_desc_t d;
    std::memset(&d, 0, sizeof(d));
    int sh = stride, sw = stride, ph = pad, pw = pad, H = x.H, W = x.W, cin = x.ld;
    int64_t sx = x.ld;
    if (geom) { W = geom[0]; sx = geom[1]; cin = geom[2]; sh = geom[3]; sw = geom[4]; ph = geom[5]; pw = geom[6]; }
    if (cin_first) cin = cin_first;             // only the first channels of every pixel (pixel stride stays x.ld)
    d.in = x.p;
    d.in_sb = (int64_t)x.H * x.W * x.ld; d.in_sy = (int64_t)x.W * x.ld; d.in_sx = sx;
    d.B = x.B; d.H = H; d.W = W; d.Cin = cin;
    d.KH = w.KH; d.KW = w.KW; d.SH = sh; d.SW = sw; d.PH = ph; d.PW = pw; d.pad_mode = pad_mode;
    d.Ho = out.H; d.Wo = out.W;
    d.wt = w.wt; d.CinP = w.CinP; d.N = w.N;
    d.a_scale = a_scale; d.a_scale_ld = a_scale_ld; d.a_shift = a_shift;
    d.bias = w.bias; d.act = act_;
    d.n_store = n_store >= 0 ? n_store : (out_coff == 0 ? out.ld - out_coff : w.N);
    if (res) { d.res = res->p; d.res_ld = res->ld; }
    if (in2) { d.in2 = in2->p; d.in2_ld = in2->ld; d.Cin2 = in2->ld; d.Cin2P = w2->CinP; d.wt2 = w2->wt; d.bias2 = w2->bias; }
    d.out = out.p; d.out_ld = out.ld; d.out_coff = out_coff; d.tile_hint = tile_hint;
    d.wt_split = w.split; d.wt_blk = w.blk;
    const float am = a_mul_override > 0.f ? a_mul_override : ((a_scale && !pre_table) ? A_MUL_GRN : A_MUL);
    d.arith = m->arith; d.a_mul = am; d.acc_mul = 1.f / (am * w.w_mul);
    if (in2) { d.wt2_split = w2->split; d.wt2_blk = w2->blk; d.acc_mul2 = 1.f / (am * w2->w_mul); }
    d.sumsq_part = sumsq;
    frame_bias(d);
    if (pre_table) d.tile_hint = (d.N % 192 == 0 ? (VS_CONV_TILE_HI | 0) : 15) | VS_CONV_PRE;   // border-class table added before bias + activation (engine.py::resblock_msg0)
    vs_conv_plan_t p;
    chk(vs_conv_plan(&d, grn_part ? grn_hw : 0, grn_c4, &p));
    d.tile_hint = p.tile_hint;
    if (p.split_k > 1) {
      d.splitk_ld = rup(w.N, 4);
      d.splitk_ws = alloc((int64_t)p.ws_slices * out.rows() * d.splitk_ld);
      d.split_k = p.split_k;
    }
    if (p.grn_fold) {       // (ABI v3) else the finish as the separate launch in front of the GEMM; the same scale values either way
      d.grn_part = grn_part; d.grn_gamma = grn_gamma; d.grn_nchunk = grn_hw / 32;
    } else if (grn_part && live()) {
      chk(vs_grn_scale_from_partials(grn_part, d.B, grn_hw, grn_c4, grn_gamma, const_cast<float*>(a_scale), a_scale_ld, st));
    }
    if (live()) chk(vs_conv_gemm(&d, st));
  }
  void layernorm(const Act& x, const float* w, const float* b, const Act& out, int act_ = VS_ACT_NONE) {
    if (live()) chk(vs_layernorm_act(x.p, x.rows(), x.C, x.ld, w, b, 1e-6f, act_, out.p, out.ld, st));
  }
  bool thin_ok(const Act& x, const RB& p, const Act* out_in) const {                          // engine.py::_thin_ok
    const int tk = p.cout == 16 ? 16 : 32;
    return (p.cout == 16 || (p.cout == 32 && m->arith == 2)) && x.ld <= tk && p.c0.CinP == tk && p.c1.CinP == tk && p.res.CinP == tk &&
           (!out_in || out_in->ld == p.cout) && vs_resblock_thin_supported(x.ld, p.cout, p.cout);
  }
  // delta != nullptr (engine.py::resblock_thin with outc): outc + tanh in the block's epilogue, the block's output is not stored
  Act resblock(const Act& x, const RB& p, const Act* out_in = nullptr, float* delta = nullptr) {  // engine.py::resblock
    if (thin_ok(x, p, out_in)) {                                                                   // engine.py::resblock_thin: t stays on chip
      Act out = delta ? Act{nullptr, x.B, x.H, x.W, p.cout, p.cout} : (out_in ? *out_in : act(x.B, x.H, x.W, p.cout));
      vs_resblock_thin_desc_t d;
      std::memset(&d, 0, sizeof(d));
      d.x = x.p; d.x_ld = x.ld; d.B = x.B; d.H = x.H; d.W = x.W; d.Cin = x.ld;
      d.w0_split = p.c0.split; d.w1_split = p.c1.split; d.wr_split = p.res.split;
      d.b0 = p.c0.bias; d.b1 = p.c1.bias; d.br = p.res.bias;
      d.arith = m->arith; d.Cout = p.cout; d.a_mul = A_MUL;
      d.acc_mul0 = 1.f / (A_MUL * p.c0.w_mul); d.acc_mul1 = 1.f / (A_MUL * p.c1.w_mul); d.acc_mulr = 1.f / (A_MUL * p.res.w_mul);
      if (delta) {
        d.outc_w = m->outc_w; d.outc_b = m->outc_b; d.out_ch = m->c.out_ch; d.use_tanh = m->c.last_tanh ? 1 : 0; d.delta = delta;
      } else {
        d.out = out.p; d.out_ld = out.ld;
      }
      if (live()) chk(vs_resblock_thin(&d, st));
      return out;
    }
    if (delta) { rc = VS_ERR_UNSUPPORTED; return Act{}; }              // (callers ask thin_ok first)
    Act t = act(x.B, x.H, x.W, p.cout);
    conv(x, p.c0, t, 1, 1, VS_PAD_ZERO, VS_ACT_RELU);
    Act out = out_in ? *out_in : act(x.B, x.H, x.W, p.cout);
    conv(t, p.c1, out, 1, 1, VS_PAD_ZERO, VS_ACT_RELU, 0, out.ld != rup(p.cout, 4) ? p.cout : -1, nullptr, &x, &p.res);
    return out;
  }
  // 1x1 GEMM on operand planes (tile code 24 / 27, gemm_pl.hip): out = act(in_pl x w + bias) (+ res), optional GRN partials / K split
  void gemm_pl(int B, int H, int W, const CW& w, const void* in_pl, const Act& out, int act_, const Act* res, float* sumsq, int split_k,
               int tile_hint, float am = A_MUL, int sumsq_hw = 0) {
    vs_conv_desc_t d;
    std::memset(&d, 0, sizeof(d));
    d.B = B; d.H = H; d.W = W; d.Cin = w.CinP; d.KH = d.KW = 1; d.SH = d.SW = 1; d.Ho = H; d.Wo = W;
    d.wt = w.wt; d.CinP = w.CinP; d.N = w.N; d.bias = w.bias; d.act = act_;
    d.wt_split = w.split; d.wt_blk = w.blk; d.arith = 2; d.a_mul = am; d.acc_mul = 1.f / (am * w.w_mul);
    d.in_pl = in_pl;
    d.out = out.p; d.out_ld = out.ld; d.n_store = out.ld;
    if (res) { d.res = res->p; d.res_ld = res->ld; }
    d.sumsq_part = sumsq;
    d.sumsq_hw = sumsq_hw;
    if (split_k > 1) {
      const int ws_ld = rup(w.N, 4);
      d.splitk_ws = alloc((int64_t)split_k * out.rows() * ws_ld);
      d.splitk_ld = ws_ld;
      d.split_k = split_k;
    }
    d.tile_hint = tile_hint;
    if (live()) chk(vs_conv_gemm(&d, st));
  }
  // one launch of the all-DMA 3x3 kernel on operand planes (tile code 22, conv3x3_pl.hip); out == nullptr: planes only
  void conv_pl(int B, int H, int W, const CW& w, const void* in_pl, void* out_pl, const Act* out, const CW* w2 = nullptr,
               const void* in2_pl = nullptr, const float* pre_table = nullptr, int64_t pre_ld = 0) {
    vs_conv_desc_t d;
    std::memset(&d, 0, sizeof(d));
    d.B = B; d.H = H; d.W = W; d.Cin = w.CinP; d.KH = d.KW = 3; d.SH = d.SW = 1; d.PH = d.PW = 1; d.pad_mode = VS_PAD_ZERO; d.Ho = H; d.Wo = W;
    d.wt = w.wt; d.CinP = w.CinP; d.N = w.N; d.bias = w.bias; d.act = VS_ACT_RELU;
    d.wt_split = w.split; d.wt_blk = w.blk; d.arith = 2; d.a_mul = A_MUL; d.acc_mul = 1.f / (A_MUL * w.w_mul);
    d.in_pl = in_pl; d.out_pl = out_pl;
    if (w2) {
      d.in2_pl = in2_pl; d.Cin2 = d.Cin2P = w2->CinP; d.wt2 = w2->wt; d.bias2 = w2->bias; d.wt2_split = w2->split; d.wt2_blk = w2->blk;
      d.acc_mul2 = 1.f / (A_MUL * w2->w_mul);
    }
    frame_bias(d);
    d.n_store = w.N;
    if (out) { d.out = out->p; d.out_ld = out->ld; d.n_store = out->ld != rup(w.N, 4) ? w.N : out->ld; }
    d.tile_hint = VS_CONV_TILE_HI | 6;
    if (pre_table) { d.a_scale = pre_table; d.a_scale_ld = pre_ld; d.tile_hint |= VS_CONV_PRE; }      // border-class table in the epilogue (first block)
    if (live()) chk(vs_conv_gemm(&d, st));
  }
  // engine.py::bottleneck_planes: ResnetBlocks j0.. from the fp32 activation x with every intermediate tensor as f16 operand planes
  Act bottleneck_planes(const Act& x, int j0, const Act* last_out, void* xpl_in = nullptr) {
    const int B = x.B, H = x.H, W = x.W, C = x.C;
    const int64_t pl_floats = x.rows() * C;               // 2 planes x rows x C f16
    void* xpl = xpl_in ? xpl_in : alloc(pl_floats);       // (the first block may hand its output over as planes already)
    void* tpl = alloc(pl_floats);
    void* ypl = alloc(pl_floats);
    if (!xpl_in && live()) chk(vs_to_planes(x.p, x.rows(), C, x.ld, A_MUL, xpl, st));
    Act out{};
    const int nb = (int)m->bottleneck.size();
    for (int j = j0; j < nb; ++j) {
      const RB& p = m->bottleneck[j];
      conv_pl(B, H, W, p.c0, xpl, tpl, nullptr);
      if (j == nb - 1) {
        out = last_out ? *last_out : act(B, H, W, C);
        conv_pl(B, H, W, p.c1, tpl, nullptr, &out, &p.res, xpl);
      } else {
        conv_pl(B, H, W, p.c1, tpl, ypl, nullptr, &p.res, xpl);
        std::swap(xpl, ypl);
      }
    }
    return out;
  }
  bool msg_vectors_ok(int B, int H, int W) const {        // engine.py::_msg_vectors_ok (the weight-only part: vs_model_create)
    const int N = m->bottleneck.empty() ? 0 : m->bottleneck[0].cout;
    return m->msgv && m->b0_table && N > 0 && W % 16 == 0 && H % 8 == 0 && (int64_t)B * (H / 8) * (W / 16) >= 128;
  }
  bool planes_ok(const Act& x, int j0) const {            // engine.py::_planes_ok
    if (m->arith != 2 || x.ld != x.C || x.C % 192 || x.H % 16 || x.W % 16 || (int64_t)x.B * (x.H / 16) * (x.W / 16) * (x.C / 192) < 200) return false;
    for (size_t j = j0; j < m->bottleneck.size(); ++j) {
      const RB& p = m->bottleneck[j];
      if (p.cout != x.C || p.c0.CinP != x.C || p.res.CinP != x.C) return false;
    }
    return j0 < (int)m->bottleneck.size();
  }
  // engine.py::embedder_forward: key frames (NHWC, ld 4, mapped to [-1,1]) -> delta [B][out_ch][S][S]
  float* embedder(const Act& x, const int32_t* msgs, int n_msgs, int& Sh, int& Sw) {
    const vs_model_cfg_t& c = m->c;
    const int B = x.B, nlev = (int)m->zc.size() - 1;
    std::vector<Act> hid;
    bool msgv = false;
    const float* up0_bias = nullptr;
    int64_t up0_fs = 0;
    hid.push_back(resblock(x, m->inc));
    for (int i = 0; i < nlev; ++i) {
      const Act src = hid.back();
      const int Ho = (src.H - 1) / 2 + 1, Wo = (src.W - 1) / 2 + 1;
      Act dwn = act(B, Ho, Wo, m->zc[i + 1]);
      conv(src, m->down_conv[i], dwn, 2, 1);
      if (i == nlev - 1) {
        msgv = msg_vectors_ok(B, Ho, Wo);         // engine.py::_msg_vectors_ok: the message channels never become a tensor, h3 = the latent alone
        Act h3 = act(B, Ho, Wo, msgv ? m->zc.back() : m->bott);
        resblock(dwn, m->down_rb[i], &h3);
        hid.push_back(h3);
      } else {
        hid.push_back(resblock(dwn, m->down_rb[i]));
      }
    }
    Act h3 = hid.back();
    float* lat = alloc((int64_t)n_msgs * c.hidden);
    if (live()) chk(vs_msg_latent(m->table, msgs, n_msgs, c.nbits, c.hidden, lat, st));
    if (!msgv && live()) chk(vs_broadcast_channels(lat, n_msgs, c.hidden, h3.p, B, h3.H * h3.W, h3.ld, m->zc.back(), st));
    Act cur = h3;
    // Upsample group k on the low-resolution map: its [x | skip] concat buffer is allocated before x's producer runs, so that the
    // producer (last bottleneck block / previous up block) writes columns [0, C) itself (engine.py::embedder_forward)
    auto fused_ok = [&](int k, int c1, int c2) -> bool {
      return m->ups[k].lowres && vs_upconv_fused_preferred(c1, c2, m->ups[k].gemm.N / 9) && m->ups[k].gemm.CinP == c1 + c2;
    };
    auto lowres_cat = [&](int k, const Act& like, Act& view) -> bool {
      if (k >= nlev || !m->ups[k].lowres) return false;
      const Act& skip = hid[nlev - k];
      if (fused_ok(k, like.C, skip.C)) return false;       // the one-kernel form reads x and skip themselves
      Act lc = act(B, like.H, like.W, like.C + skip.C);
      view = Act{lc.p, B, like.H, like.W, like.C, lc.ld};
      return true;
    };
    void* cur_pl = nullptr;
    for (int j = 0; j < c.num_blocks; ++j) {
      Act view{};
      const bool direct = j == c.num_blocks - 1 && lowres_cat(0, cur, view);
      const RB& rb = m->bottleneck[j];
      if (j == 0 && msgv) {                                                      // engine.py::resblock_msg0_vec
        const int nx = m->b0_msg.N, N = rb.cout, nlat = m->zc.back();
        Act P = act(n_msgs, 1, 1, nx);
        conv(Act{lat, n_msgs, 1, 1, c.hidden, c.hidden}, m->b0_msg, P);
        float* table = alloc((int64_t)n_msgs * 9 * N);
        if (live()) chk(vs_msg_pre_rows(P.p, nx, n_msgs, N, table, st));
        const int64_t fs = n_msgs == 1 ? 0 : nx;
        up0_bias = P.p + m->msgv_off_up; up0_fs = fs;
        if (!planes_ok(Act{nullptr, B, h3.H, h3.W, N, N}, 1)) {                  // per-conv path: both convs on the wave-specialised kernel, named by tile
          const int tile = N % 192 == 0 ? (VS_CONV_TILE_HI | 0) : 15;
          Act t = act(B, h3.H, h3.W, N);
          conv(h3, m->b0_lat, t, 1, 1, VS_PAD_ZERO, VS_ACT_RELU, 0, -1, nullptr, nullptr, nullptr, table, n_msgs == 1 ? 0 : 9 * (int64_t)N, nullptr,
               nullptr, nullptr, nlat, true);
          Act out = act(B, h3.H, h3.W, N);
          fb_bias2 = P.p + m->msgv_off_res; fb_bias2_fs = fs;
          conv(t, rb.c1, out, 1, 1, VS_PAD_ZERO, VS_ACT_RELU, 0, -1, nullptr, &h3, &m->b0_res_lat, nullptr, 0, nullptr, nullptr, nullptr, 0, false, 0.f,
               nullptr, nullptr, 0, 0, tile);
          cur = out;
          continue;
        }
        void* latpl = alloc(h3.rows() * nlat);
        void* tpl = alloc(h3.rows() * N);
        void* xpl = alloc(h3.rows() * N);
        if (live()) chk(vs_to_planes(h3.p, h3.rows(), nlat, h3.ld, A_MUL, latpl, st));
        conv_pl(B, h3.H, h3.W, m->b0_lat, latpl, tpl, nullptr, nullptr, nullptr, table, n_msgs == 1 ? 0 : 9 * (int64_t)N);
        fb_bias2 = P.p + m->msgv_off_res; fb_bias2_fs = fs;                      // res_conv's message part (+ its bias), one vector per frame
        conv_pl(B, h3.H, h3.W, rb.c1, tpl, xpl, nullptr, &m->b0_res_lat, latpl);
        cur = Act{nullptr, B, h3.H, h3.W, N, N};
        cur_pl = xpl;
        continue;
      }
      if (j == 0 && !direct && m->b0_table && h3.ld == h3.C && rb.c0.CinP == h3.C && h3.W % 16 == 0 && h3.H % 8 == 0 &&
          (int64_t)B * (h3.H / 8) * (h3.W / 16) >= 128) {                        // engine.py::resblock_msg0
        const int N9 = m->b0_msg.N, N = rb.cout;             // (N9 > 9 N: the rows of the per-frame vectors, unused on this path)
        Act P = act(n_msgs, 1, 1, N9);
        conv(Act{lat, n_msgs, 1, 1, c.hidden, c.hidden}, m->b0_msg, P);
        float* table = alloc((int64_t)n_msgs * 9 * N);
        if (live()) chk(vs_msg_pre_rows(P.p, N9, n_msgs, N, table, st));
        const Act nxt{nullptr, B, h3.H, h3.W, N, N};
        if (c.num_blocks > 1 && N == h3.C && m->zc.back() % 16 == 0 && planes_ok(nxt, 1)) {
          // engine.py::resblock_msg0(planes_out=True), round 5: the block on the all-DMA planes kernel, output handed to the chain as planes
          const int nlat = m->zc.back();
          void* latpl = alloc(h3.rows() * nlat);
          void* h3pl = alloc(h3.rows() * h3.C);
          void* tpl = alloc(h3.rows() * N);
          void* xpl = alloc(h3.rows() * N);
          if (live()) {
            chk(vs_to_planes(h3.p, h3.rows(), nlat, h3.ld, A_MUL, latpl, st));
            chk(vs_to_planes(h3.p, h3.rows(), h3.C, h3.ld, A_MUL, h3pl, st));
          }
          conv_pl(B, h3.H, h3.W, m->b0_lat, latpl, tpl, nullptr, nullptr, nullptr, table, n_msgs == 1 ? 0 : 9 * (int64_t)N);
          conv_pl(B, h3.H, h3.W, rb.c1, tpl, xpl, nullptr, &rb.res, h3pl);
          cur = nxt;
          cur_pl = xpl;
          continue;
        }
        Act t = act(B, h3.H, h3.W, N);
        conv(h3, m->b0_lat, t, 1, 1, VS_PAD_ZERO, VS_ACT_RELU, 0, -1, nullptr, nullptr, nullptr, table, n_msgs == 1 ? 0 : 9 * (int64_t)N, nullptr,
             nullptr, nullptr, m->zc.back(), true);
        Act out = act(B, h3.H, h3.W, N);
        conv(t, rb.c1, out, 1, 1, VS_PAD_ZERO, VS_ACT_RELU, 0, -1, nullptr, &h3, &rb.res);
        cur = out;
        continue;
      }
      if (j >= 1 && planes_ok(cur, j)) {                 // the rest of the chain on operand planes
        Act v2 = view;
        const bool d2 = j == c.num_blocks - 1 ? direct : lowres_cat(0, cur, v2);
        cur = bottleneck_planes(cur, j, d2 ? &v2 : nullptr, cur_pl);
        break;
      }
      cur = resblock(cur, rb, direct ? &view : nullptr);
    }
    for (int k = 0; k < nlev; ++k) {                   // skips are popped deepest first; the first one is the [latent | message] map itself
      const Act skip = hid.back();
      hid.pop_back();
      const Up& up = m->ups[k];
      Act ln{};
      if (up.lowres && cur.ld == cur.C && fused_ok(k, cur.C, skip.C)) {
        const int co = up.gemm.N / 9;
        ln = act(B, 2 * cur.H, 2 * cur.W, co);
        if (live()) chk(vs_upconv_fused(cur.p, cur.C, cur.ld, skip.p, skip.C, skip.ld, 0.70710678118654752440f, up.gemm.split, B, cur.H, cur.W, co,
                                        up.lnw, up.lnb, 1e-6f, VS_ACT_RELU, ln.p, ln.ld, m->arith, A_MUL, 1.f / (A_MUL * up.gemm.w_mul), st));
      } else if (up.lowres) {
        const int co = up.gemm.N / 9;
        const bool direct = cur.ld == cur.C + skip.C;
        Act lc = direct ? Act{cur.p, B, cur.H, cur.W, cur.C + skip.C, cur.ld} : act(B, cur.H, cur.W, cur.C + skip.C);
        if (live()) chk(vs_cat2_scale(direct ? nullptr : cur.p, cur.C, cur.ld, skip.p, skip.C, skip.ld, 0.70710678118654752440f, lc.rows(), lc.p, lc.ld, st));
        Act z = act(B, lc.H, lc.W, 9 * co);
        if (k == 0 && up0_bias) {               // [x | latent skip]: the message-skip columns arrive as one bias vector per frame
          fb_bias = up0_bias; fb_bias_fs = up0_fs;
          conv(lc, m->up0_xl, z);
        } else {
          conv(lc, up.gemm, z);
        }
        ln = act(B, 2 * lc.H, 2 * lc.W, co);
        if (live()) chk(vs_upconv_gather_ln(z.p, z.ld, B, lc.H, lc.W, co, up.lnw, up.lnb, 1e-6f, VS_ACT_RELU, ln.p, ln.ld, st));
      } else {
        Act cat = act(B, 2 * cur.H, 2 * cur.W, cur.C + skip.C);
        if (live()) chk(vs_upcat2x(cur.p, cur.C, cur.ld, skip.p, skip.C, skip.ld, 0.70710678118654752440f, B, cur.H, cur.W, cat.p, cat.ld, st));
        Act cv = act(B, cat.H, cat.W, up.conv.N);
        conv(cat, up.conv, cv, 1, 1, VS_PAD_REFLECT);
        ln = act(B, cat.H, cat.W, up.conv.N);
        layernorm(cv, up.lnw, up.lnb, ln, VS_ACT_RELU);
      }
      Act view{};
      const bool direct = lowres_cat(k + 1, Act{nullptr, B, ln.H, ln.W, up.rb.cout, 0}, view);
      if (k == nlev - 1 && !direct && up.rb.cout == 16 && c.out_ch <= 4 && m->zc[0] == 16 && thin_ok(ln, up.rb, nullptr)) {
        // engine.py: outc + tanh in the last block's epilogue (its 16-channel output was written to be read once); same bits as the two launches
        float* delta = alloc((int64_t)B * c.out_ch * ln.H * ln.W);
        resblock(ln, up.rb, nullptr, delta);
        Sh = ln.H; Sw = ln.W;
        return delta;
      }
      cur = resblock(ln, up.rb, direct ? &view : nullptr);
    }
    float* delta = alloc((int64_t)B * c.out_ch * cur.H * cur.W);
    if (live()) chk(vs_outc_tanh(cur.p, (int64_t)cur.H * cur.W, B, cur.C, cur.ld, m->outc_w, m->outc_b, c.out_ch, c.last_tanh ? 1 : 0, delta, st));
    Sh = cur.H; Sw = cur.W;
    return delta;
  }
  // engine.py::extractor_forward: frames (NHWC ld 4, mapped to [-1,1]) -> logits [B][1+nbits]
  void extractor(const Act& x, float* logits) {
    const vs_model_cfg_t& c = m->c;
    const int B = x.B, s = c.stem_stride;
    int Ho = (x.H - 4) / s + 1, Wo = (x.W - 4) / s + 1;
    Act cur = act(B, Ho, Wo, c.dims[0], xld(c.dims[0]));
    const int co = c.dims[0];
    const bool stem_fused = vs_debug_get(VS_DBG_STEM_FUSED) == 1;      // (measured neutral: opt-in, as engine.py)
    if (stem_fused && x.ld == 4 && cur.ld == co && (co == 64 || co == 96 || co == 128) && m->stem.bias) {
      // engine.py (round 6): patchify conv + LayerNorm in one kernel on the vector ALUs
      if (live()) chk(vs_stem_conv_ln(x.p, B, x.H, x.W, s, m->stem.wt, m->stem.bias, m->stem_lnw, m->stem_lnb, 1e-6f, co, cur.p, cur.ld, st));
    } else {
      Act t = act(B, Ho, Wo, c.dims[0]);
      { const int geom[7] = {Wo, s * 4, 16, s, 1, 0, 0}; conv(x, m->stem, t, 1, 0, VS_PAD_ZERO, VS_ACT_NONE, 0, -1, nullptr, nullptr, nullptr, nullptr, 0, nullptr, geom); }
      layernorm(t, m->stem_lnw, m->stem_lnb, cur);
    }
    for (int sti = 0; sti < 4; ++sti) {
      if (sti > 0) {
        const Down& dn = m->down[sti - 1];
        Ho = cur.H / 2; Wo = cur.W / 2;
        if (cur.ld == cur.C && cur.C % 8 == 0 && dn.gemm.CinP == 4 * cur.C && Ho > 0 && Wo > 0) {
          // engine.py (round 6): LayerNorm straight into the 2 x 2 patch matrix, the conv as a dense GEMM
          Act lnp = act(B, Ho, Wo, 4 * cur.C, 4 * cur.C);
          Act nxt = act(B, Ho, Wo, c.dims[sti], xld(c.dims[sti]));
          if (live()) chk(vs_layernorm_patch2x2(cur.p, B, cur.H, cur.W, cur.C, cur.ld, dn.lnw, dn.lnb, 1e-6f, lnp.p, st));
          conv(lnp, dn.gemm, nxt);
          cur = nxt;
        } else {
          Act ln = act(B, cur.H, cur.W, cur.C, cur.ld);
          layernorm(cur, dn.lnw, dn.lnb, ln);
          Act nxt = act(B, Ho, Wo, c.dims[sti], xld(c.dims[sti]));
          const int geom[7] = {Wo, 2 * ln.ld, 2 * ln.ld, 2, 1, 0, 0};
          conv(ln, dn.conv, nxt, 1, 0, VS_PAD_ZERO, VS_ACT_NONE, 0, -1, nullptr, nullptr, nullptr, nullptr, 0, nullptr, geom);
          cur = nxt;
        }
      }
      const int Cc = c.dims[sti], HW = cur.H * cur.W;
      Act tn = act(B, cur.H, cur.W, Cc, xld(Cc));
      Act hh = act(B, cur.H, cur.W, 4 * Cc, xld(4 * Cc));
      float* part = alloc((int64_t)((HW + 63) / 64) * B * 4 * Cc);
      float* part32 = alloc((int64_t)B * ((HW + 31) / 32) * 4 * Cc);
      float* scale = alloc((int64_t)B * hh.ld + 16);
      float* parts = (HW % 32 != 0 && HW >= 32) ? alloc((((int64_t)B * HW + 31) / 32) * 2 * 4 * Cc) : nullptr;
      // engine.py::_extractor_forward: which of the two GEMMs run on operand planes, pwconv2's K slices and its 128 x 96 form
      const int64_t rows = cur.rows();
      const CW& pw1w = m->stages[sti].empty() ? m->stem : m->stages[sti][0].pw1;
      vs_cnx_stage_plan_t sp;
      chk(vs_cnx_stage_plan(rows, HW, Cc, hh.ld, pw1w.CinP, m->arith, 0, &sp));
      const bool pl1 = sp.pl1 && !m->stages[sti].empty(), pl2 = sp.pl2;
      // engine.py::_extractor_forward: pwconv1 -> GELU -> GRN -> pwconv2 with h on chip (statistics pass, scale, apply pass in place on cur)
      const bool fused = m->arith == 2 && !m->stages[sti].empty() && m->stages[sti][0].fuse && pw1w.CinP == Cc && vs_cnx_block_supported(Cc, rows, HW);
      void* tnpl = (pl1 || fused) ? alloc(rows * pw1w.CinP) : nullptr;
      void* hpl = pl2 ? alloc(rows * hh.ld) : nullptr;
      for (const Blk& blk : m->stages[sti]) {
        if (fused && blk.fuse) {
          if (live()) {
            chk(vs_dwconv7_ln_planes(cur.p, B, cur.H, cur.W, Cc, cur.ld, blk.wdw, blk.bdw, blk.lnw, blk.lnb, 1e-6f, A_MUL, pw1w.CinP, tnpl, st));
            const float am1 = 1.f / (A_MUL * blk.fm1), am2 = 1.f / (A_MUL_GRN * blk.fm2);
            chk(vs_cnx_block(tnpl, blk.fuse, Cc, rows, HW, 1, am1, am2, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, part32, st));
            chk(vs_grn_scale_from_partials(part32, B, HW, 4 * Cc, blk.gamma, scale, hh.ld, st));
            chk(vs_cnx_block(tnpl, blk.fuse, Cc, rows, HW, 0, am1, am2, scale, hh.ld, blk.pw2.bias, cur.p, cur.ld, cur.p, cur.ld, nullptr, st));
          }
          continue;
        }
        if (pl1) {
          if (live()) chk(vs_dwconv7_ln_planes(cur.p, B, cur.H, cur.W, Cc, cur.ld, blk.wdw, blk.bdw, blk.lnw, blk.lnb, 1e-6f, A_MUL, pw1w.CinP, tnpl, st));
        } else if (live()) {
          chk(vs_dwconv7_ln(cur.p, B, cur.H, cur.W, Cc, cur.ld, blk.wdw, blk.bdw, blk.lnw, blk.lnb, 1e-6f, tn.p, tn.ld, st));
        }
        if (HW % 32 == 0) {
          if (pl1) gemm_pl(B, cur.H, cur.W, blk.pw1, tnpl, hh, VS_ACT_GELU, nullptr, part32, 1, sp.tile1);
          else conv(tn, blk.pw1, hh, 1, 0, VS_PAD_ZERO, VS_ACT_GELU, 0, -1, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, part32);
          // (the finish is deferred to pwconv2's conv() where that launch can fold it, engine.py)
          if (!(HW % 64 == 0 && !pl2) && live()) chk(vs_grn_scale_from_partials(part32, B, HW, 4 * Cc, blk.gamma, scale, hh.ld, st));
        } else if (pl1 && HW >= 32) {      // engine.py (round 6): straddling 32-row-group partials from the planes GEMM's epilogue
          gemm_pl(B, cur.H, cur.W, blk.pw1, tnpl, hh, VS_ACT_GELU, nullptr, parts, 1, sp.tile1, A_MUL, HW);
          if (live()) chk(vs_grn_scale_from_straddle_partials(parts, B, HW, 4 * Cc, blk.gamma, scale, hh.ld, st));
        } else {
          if (pl1) gemm_pl(B, cur.H, cur.W, blk.pw1, tnpl, hh, VS_ACT_GELU, nullptr, nullptr, 1, sp.tile1);
          else conv(tn, blk.pw1, hh, 1, 0, VS_PAD_ZERO, VS_ACT_GELU);
          if (live()) chk(vs_grn_scale(hh.p, B, HW, 4 * Cc, hh.ld, blk.gamma, part, scale, st));
        }
        if (pl2) {
          if (live()) chk(vs_to_planes_affine(hh.p, hh.rows(), hh.ld, hh.ld, A_MUL_GRN, scale, hh.ld, blk.beta, HW, hpl, st));
          gemm_pl(B, cur.H, cur.W, blk.pw2, hpl, cur, VS_ACT_NONE, &cur, nullptr, sp.sk2, sp.tile2, A_MUL_GRN);
        } else if (HW % 64 == 0) {
          const bool defer = HW % 32 == 0;
          conv(hh, blk.pw2, cur, 1, 0, VS_PAD_ZERO, VS_ACT_NONE, 0, -1, &cur, nullptr, nullptr, scale, hh.ld, blk.beta, nullptr, nullptr, 0, false, 0.f,
               defer ? part32 : nullptr, blk.gamma, HW, 4 * Cc, sp.pw2_narrow ? (VS_CONV_TILE_HI | 10) : 0);
        } else {
          if (live()) chk(vs_grn_apply(hh.p, B, HW, 4 * Cc, hh.ld, scale, hh.ld, blk.beta, st));
          conv(hh, blk.pw2, cur, 1, 0, VS_PAD_ZERO, VS_ACT_NONE, 0, -1, &cur, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, false, A_MUL_GRN);
        }
      }
    }
    Act hc = act(B, cur.H, cur.W, c.dims[3]);
    if (cur.rows() <= 4096 && cur.H > 1 && cur.W > 1 && m->head.CinP == cur.ld) {       // engine.py::extractor_forward
      Act cols{alloc(cur.rows() * 9 * cur.ld), B, cur.H, cur.W, 9 * cur.ld, 9 * cur.ld};
      if (live()) chk(vs_im2col3x3(cur.p, B, cur.H, cur.W, cur.ld, VS_PAD_REFLECT, cols.p, st));
      conv(cols, m->head_gemm, hc);
    } else {
      conv(cur, m->head, hc, 1, 1, VS_PAD_REFLECT);
    }
    Act hl = act(B, cur.H, cur.W, c.dims[3]);
    layernorm(hc, m->head_lnw, m->head_lnb, hl, VS_ACT_GELU);
    if (live()) chk(vs_pool_linear(hl.p, B, hl.H * hl.W, hl.C, hl.ld, m->lin_w, m->lin_b, c.nbits + 1, logits, st));
  }
  // model.py::_embed_frames_eager
  // io: 0 = fp32 NCHW, 3 = the YUV surface `ysrc` (io_u8 = 2 arrives here as a contiguous nv12 surface), 4 = the packed RGB surface `psrc`,
  // 5 = the half-precision surface `hsrc`, any other value = RGB24
  void resize(const void* imgs, int io, int F, int H, int W, int S, int antialias, float* rgb, float mul, float add, float* key, int step,
              const float* ymat) {
    if (!live()) return;
    const bool u8 = io != 0;
    if (io == 3) chk(vs_resize_pre_yuv(ysrc, F, H, W, ydec, S, S, antialias, rgb, mul, add, key, step, ymat, st));
    else if (io == 4) chk(vs_resize_pre_rgb(psrc, F, H, W, S, S, antialias, rgb, mul, add, key, step, ymat, st));
    else if (io == 5) chk(vs_resize_pre_half(hsrc, F, H, W, S, S, antialias, rgb, mul, add, key, step, ymat, st));
    else if (u8) chk(vs_resize_pre_u8(static_cast<const unsigned char*>(imgs), F, H, W, S, S, antialias, rgb, mul, add, key, step, ymat, st));
    else chk(vs_resize_pre(static_cast<const float*>(imgs), F, 3, H, W, S, S, antialias, rgb, mul, add, key, step, ymat, st));
  }
  void embed(const void* imgs, int io, const int32_t* msgs, int n_msgs, int F, int H, int W, int step, int video_mode, int lowres, int antialias,
             void* out, float* preds_w) {
    const vs_model_cfg_t& c = m->c;
    const int S = c.img_size, nk = (F + step - 1) / step;
    const bool att = c.attenuate != 0;
    Act rgb{nullptr, F, S, S, 3, 4}, key = act(nk, S, S, c.in_ch, 4);
    if (att && lowres) rgb = act(F, S, S, 3, 4);
    resize(imgs, io, F, H, W, S, antialias, (att && lowres) ? rgb.p : nullptr, 1.0f, 0.0f, key.p, step, c.yuv ? m->ymat : nullptr);
    int Sh = 0, Sw = 0;
    float* delta = embedder(key, msgs, n_msgs, Sh, Sw);
    float* hmap = nullptr;
    if (att && lowres) {
      hmap = alloc((int64_t)F * S * S);
      if (live()) chk(vs_jnd_heatmap(rgb.p, F, S, S, (int64_t)S * S * 4, 1, (int64_t)S * 4, 4, m->taps43, hmap, st));
    }
    if (io == 3) {
      vs_tail_yuv_desc_t n;
      std::memset(&n, 0, sizeof(n));
      n.src = *ysrc; n.dst = *ydst; n.preds_w = preds_w; n.delta = delta; n.hmap_lowres = hmap; n.taps43 = m->taps43;
      n.F = F; n.H = H; n.W = W; n.S_h = Sh; n.S_w = Sw; n.Cd = c.out_ch;
      n.step = step; n.video_mode = video_mode; n.total_key = nk;
      n.attenuate = att ? 1 : 0; n.clamp = c.clamp; n.antialias = antialias;
      n.scaling_i = c.scaling_i; n.scaling_w = c.scaling_w;
      std::memcpy(n.yuv2rgb12, ydec, sizeof(n.yuv2rgb12));
      std::memcpy(n.rgb2yuv12, yenc, sizeof(n.rgb2yuv12));
      if (live()) chk(vs_embed_tail_yuv(&n, st));
      return;
    }
    if (io == 4) {
      vs_tail_rgb_desc_t n;
      std::memset(&n, 0, sizeof(n));
      n.src = *psrc; n.dst = *pdst; n.preds_w = preds_w; n.delta = delta; n.hmap_lowres = hmap; n.taps43 = m->taps43;
      n.F = F; n.H = H; n.W = W; n.S_h = Sh; n.S_w = Sw; n.Cd = c.out_ch;
      n.step = step; n.video_mode = video_mode; n.total_key = nk;
      n.attenuate = att ? 1 : 0; n.clamp = c.clamp; n.antialias = antialias;
      n.scaling_i = c.scaling_i; n.scaling_w = c.scaling_w;
      if (live()) chk(vs_embed_tail_rgb(&n, st));
      return;
    }
    if (io == 5) {
      vs_tail_half_desc_t n;
      std::memset(&n, 0, sizeof(n));
      n.src = *hsrc; n.dst = *hdst; n.preds_w = preds_w; n.delta = delta; n.hmap_lowres = hmap; n.taps43 = m->taps43;
      n.F = F; n.H = H; n.W = W; n.S_h = Sh; n.S_w = Sw; n.Cd = c.out_ch;
      n.step = step; n.video_mode = video_mode; n.total_key = nk;
      n.attenuate = att ? 1 : 0; n.clamp = c.clamp; n.antialias = antialias;
      n.scaling_i = c.scaling_i; n.scaling_w = c.scaling_w;
      if (live()) chk(vs_embed_tail_half(&n, st));
      return;
    }
    const bool u8 = io != 0;
    vs_tail_desc_t d;
    std::memset(&d, 0, sizeof(d));
    d.imgs = imgs; d.out = out; d.preds_w = preds_w; d.delta = delta; d.hmap_lowres = hmap; d.taps43 = m->taps43;
    d.F = F; d.H = H; d.W = W; d.S_h = Sh; d.S_w = Sw; d.Cd = c.out_ch;
    d.step = step; d.video_mode = video_mode; d.total_key = nk;
    d.attenuate = att ? 1 : 0; d.clamp = c.clamp; d.antialias = antialias;
    d.scaling_i = c.scaling_i; d.scaling_w = c.scaling_w;
    d.io_u8 = u8 ? 1 : 0;
    if (psnr) {           // model.py::embed_psnr on one chunk: energy pass -> strengths -> scaled tail, three launches on `st`
      const int64_t np = vs_tail_energy_partial_doubles(F, H, W);
      double* partials = reinterpret_cast<double*>(alloc(2 * np));
      double* energy = reinterpret_cast<double*>(alloc(2 * (int64_t)F));
      if (live()) chk(vs_embed_tail_energy(&d, partials, energy, st));
      if (live()) chk(vs_psnr_scale(energy, F, H, W, psnr->per_clip, psnr->target_db, psnr->max_scale, psnr->scale_out, st));
      if (live()) chk(vs_embed_tail_scaled(&d, psnr->scale_out, st));
      return;
    }
    if (live()) chk(vs_embed_tail(&d, st));
  }
  void detect(const void* imgs, int io, int F, int H, int W, int antialias, float* logits) {
    const int S = m->c.img_size;
    Act rgb = act(F, S, S, 3, 4);
    resize(imgs, io, F, H, W, S, antialias, rgb.p, 2.0f, -1.0f, nullptr, 1, nullptr);
    extractor(rgb, logits);
  }
};

}  // namespace

static void yuv420_default_color(int depth, float* yuv2rgb12, float* rgb2yuv12);
static void nv12_default_color(float* yuv2rgb12, float* rgb2yuv12) { yuv420_default_color(8, yuv2rgb12, rgb2yuv12); }

extern "C" int vs_model_create(const vs_model_cfg_t* cfg, const vs_tensor_t* tensors, int ntensors, vs_model_t** out) {
  VS_REQUIRE(cfg && tensors && ntensors > 0 && out);
  VS_REQUIRE(cfg->nlev >= 1 && cfg->nlev <= 7 && cfg->num_blocks >= 0 && (cfg->out_ch == 1 || cfg->out_ch == 3) && cfg->nbits > 0 && cfg->nbits <= 1024);
  std::map<std::string, HostT> sd;
  for (int i = 0; i < ntensors; ++i) {
    VS_REQUIRE(tensors[i].name && tensors[i].data && tensors[i].numel > 0);
    sd[tensors[i].name] = HostT{tensors[i].data, tensors[i].numel};
  }
  vs_model* m = new vs_model();
  m->c = *cfg;
  m->arith = cfg->arith == 2 || cfg->arith == 3 ? cfg->arith : vs_default_arith();
  nv12_default_color(m->yuv2rgb12, m->rgb2yuv12);
  for (int i = 0; i <= cfg->nlev; ++i) {
    m->zc.push_back(cfg->zc[i]);
    if (cfg->zc[i] % 4) { delete m; return VS_ERR_UNSUPPORTED; }
  }
  m->bott = m->zc.back() + cfg->hidden;
  Packer P{m, sd};
  const std::string u = "embedder.unet";
  P.resblock(m->inc, u + ".inc", cfg->in_ch);
  const int nlev = cfg->nlev;
  m->down_conv.resize(nlev); m->down_rb.resize(nlev); m->ups.resize(nlev); m->bottleneck.resize(cfg->num_blocks);
  for (int i = 0; i < nlev; ++i) {
    const std::string p = u + ".downs." + std::to_string(i);
    P.conv(m->down_conv[i], p + ".down.weight", m->zc[i], 3, 3, rup(m->zc[i], 4), nullptr, nullptr, p + ".down.bias");
    P.resblock(m->down_rb[i], p + ".conv", m->zc[i + 1]);
  }
  std::vector<float> w0, b0, wres0, wup0;             // packed host weights of the layers that read the message channels
  const int nlat = m->zc.back(), hidden = cfg->hidden;
  for (int j = 0; j < cfg->num_blocks; ++j) {
    const bool table = j == 0 && nlat % 16 == 0 && hidden % 32 == 0 && m->bott % 16 == 0;
    P.resblock(m->bottleneck[j], u + ".bottleneck.model." + std::to_string(j), m->bott, table ? &w0 : nullptr, table ? &b0 : nullptr,
               table ? &wres0 : nullptr);
  }
  std::vector<int> zz(m->zc.begin(), m->zc.end() - 1);
  zz.push_back(m->bott);
  for (int k = 0; k < nlev; ++k) {
    const int i = nlev - 1 - k;
    const int cin = 2 * zz[i + 1], cout = zz[i];
    const std::string p = u + ".ups." + std::to_string(k);
    m->ups[k].lowres = vs_upconv_supported(cout) != 0;
    if (m->ups[k].lowres) P.upconv9(m->ups[k].gemm, p + ".up.upsample_block.2.weight", cin, cout, k == 0 ? &wup0 : nullptr);
    else P.conv(m->ups[k].conv, p + ".up.upsample_block.2.weight", cin, 3, 3, rup(cin, 4), nullptr, nullptr, "");
    m->ups[k].lnw = P.vec(p + ".up.upsample_block.3.weight");
    m->ups[k].lnb = P.vec(p + ".up.upsample_block.3.bias");
    P.resblock(m->ups[k].rb, p + ".conv", cout);
  }
  if (!w0.empty() && m->bottleneck[0].cout >= 128) {
    const RB& rb0 = m->bottleneck[0];
    const int n = rb0.cout;
    const HostT& bres = P.get(u + ".bottleneck.model.0.res_conv.bias");
    const CW* gm = nlev > 0 && m->ups[0].lowres ? &m->ups[0].gemm : nullptr;
    // engine.py::_msg_vectors_ok, the part that depends on the weights alone
    if (cfg->num_blocks > 1 && gm && !wres0.empty() && !wup0.empty() && bres.p && bres.n == n && n == m->bott && n % 192 == 0 && rb0.res.CinP == m->bott &&
        gm->CinP == n + m->bott && (n + nlat) % 32 == 0 && gm->N % 4 == 0) {
      const int cx = gm->CinP - nlat - hidden, nu = gm->N;
      std::vector<float> extra((size_t)(n + nu) * hidden), eb((size_t)n + nu, 0.f), wrl((size_t)n * nlat), wxl((size_t)nu * (cx + nlat));
      for (int o = 0; o < n; ++o) {
        const float* src = &wres0[(size_t)o * rb0.res.CinP];
        std::copy(src, src + nlat, &wrl[(size_t)o * nlat]);
        std::copy(src + nlat, src + nlat + hidden, &extra[(size_t)o * hidden]);
        eb[o] = bres.p[o];
      }
      for (int o = 0; o < nu; ++o) {
        const float* src = &wup0[(size_t)o * gm->CinP];
        std::copy(src, src + cx + nlat, &wxl[(size_t)o * (cx + nlat)]);
        for (int c = 0; c < hidden; ++c) extra[(size_t)(n + o) * hidden + c] = src[cx + nlat + c] * 0.70710678118654752440f;
      }
      P.msg_table_convs(m->b0_lat, m->b0_msg, w0, b0, n, rb0.c0.CinP, nlat, hidden, &extra, &eb);
      m->b0_res_lat.N = n; m->b0_res_lat.KH = m->b0_res_lat.KW = 1; m->b0_res_lat.CinP = nlat;
      P.finish(m->b0_res_lat, wrl, {}, false);
      m->up0_xl.N = nu; m->up0_xl.KH = m->up0_xl.KW = 1; m->up0_xl.CinP = cx + nlat;
      P.finish(m->up0_xl, wxl, {}, false);
      m->msgv = true; m->msgv_off_res = 9 * n; m->msgv_off_up = 10 * n;
    } else {
      P.msg_table_convs(m->b0_lat, m->b0_msg, w0, b0, n, rb0.c0.CinP, nlat, hidden);
    }
    m->b0_table = true;
  }
  m->outc_w = P.vec(u + ".outc.weight");
  m->outc_b = P.vec(u + ".outc.bias");
  m->table = P.vec(u + ".msg_processor.msg_embeddings.weight");
  // extractor
  const std::string cn = "detector.convnext";
  P.patch_conv(m->stem, cn + ".downsample_layers.0.0.weight", 3, 4, 4, cn + ".downsample_layers.0.0.bias");
  m->stem_lnw = P.vec(cn + ".downsample_layers.0.1.weight");
  m->stem_lnb = P.vec(cn + ".downsample_layers.0.1.bias");
  for (int i = 0; i < 3; ++i) {
    const std::string p = cn + ".downsample_layers." + std::to_string(i + 1);
    m->down[i].lnw = P.vec(p + ".0.weight");
    m->down[i].lnb = P.vec(p + ".0.bias");
    P.patch_conv(m->down[i].conv, p + ".1.weight", cfg->dims[i], 2, xld(cfg->dims[i]), p + ".1.bias", &m->down[i].gemm);
  }
  for (int s = 0; s < 4; ++s) {
    const int Cc = cfg->dims[s], ld = xld(Cc), ld4 = xld(4 * Cc);
    m->stages[s].resize(cfg->depths[s]);
    for (int j = 0; j < cfg->depths[s]; ++j) {
      const std::string p = cn + ".stages." + std::to_string(s) + "." + std::to_string(j);
      Blk& b = m->stages[s][j];
      const HostT& dw = P.get(p + ".dwconv.weight");
      if (dw.p) {
        std::vector<float> wdw((size_t)49 * ld, 0.f);
        for (int c2 = 0; c2 < Cc; ++c2)
          for (int t = 0; t < 49; ++t) wdw[(size_t)t * ld + c2] = dw.p[(size_t)c2 * 49 + t];
        b.wdw = P.upload(wdw);
      }
      b.bdw = P.vec(p + ".dwconv.bias", ld);
      b.lnw = P.vec(p + ".norm.weight", ld);
      b.lnb = P.vec(p + ".norm.bias", ld);
      b.gamma = P.vec(p + ".grn.gamma");
      b.beta = P.vec(p + ".grn.beta", rup(ld4, 16));
      P.conv(b.pw1, p + ".pwconv1.weight", Cc, 1, 1, ld, nullptr, nullptr, p + ".pwconv1.bias");
      P.conv(b.pw2, p + ".pwconv2.weight", 4 * Cc, 1, 1, ld4, nullptr, nullptr, p + ".pwconv2.bias");
      if (s < 2 && (Cc == 96 || Cc == 192) && m->arith == 2)      // engine.py::_pack_extractor: the fused block kernel of stages 0 / 1
        b.fuse = P.cnx_image(P.get(p + ".pwconv1.weight"), P.get(p + ".pwconv1.bias"), P.get(p + ".pwconv2.weight"), P.get(p + ".grn.beta"), Cc,
                             b.fm1, b.fm2);
    }
  }
  const std::string pd = "detector.pixel_decoder";
  P.conv(m->head, pd + ".output_upscaling.0.upsample_block.2.weight", cfg->dims[3], 3, 3, xld(cfg->dims[3]), nullptr, nullptr, "", &m->head_gemm);
  m->head_lnw = P.vec(pd + ".output_upscaling.0.upsample_block.3.weight");
  m->head_lnb = P.vec(pd + ".output_upscaling.0.upsample_block.3.bias");
  m->lin_w = P.vec(pd + ".linear.weight");
  m->lin_b = P.vec(pd + ".linear.bias");
  const HostT& M = P.get("rgb2yuv.M", !cfg->yuv);
  if (M.p) for (int i = 0; i < 3; ++i) m->ymat[i] = M.p[i];
  const bool noatt = !cfg->attenuate;
  const HostT &tl = P.get("attenuation.conv_lum.weight", noatt), &tx = P.get("attenuation.conv_x.weight", noatt), &ty = P.get("attenuation.conv_y.weight", noatt);
  if (tl.p && tx.p && ty.p) {
    for (int i = 0; i < 25; ++i) m->taps43[i] = tl.p[i];
    for (int i = 0; i < 9; ++i) { m->taps43[25 + i] = tx.p[i]; m->taps43[34 + i] = ty.p[i]; }
  }
  if (P.fail) {
    for (void* d : m->dev) (void)hipFree(d);
    delete m;
    return VS_ERR_BAD_ARG;       // a tensor of the state_dict is missing (or the device ran out of memory)
  }
  *out = m;
  return VS_OK;
}

// BT.709 limited range, the expressions of videoseal_amd/yuv420.py::color_affine (nv12.py's is its depth 8) in the same order: the
// forward affine in double, its inverse by cofactors in double (no contraction into fused multiply-adds: numpy has none), both rounded to
// fp32 once -- the same 24 floats, bit for bit
static void yuv420_default_color(int depth, float* yuv2rgb12, float* rgb2yuv12) {
#pragma clang fp contract(off)
  const double kr = 0.2126, kb = 0.0722, kg = 1.0 - kr - kb, ys = depth == 10 ? 876.0 : 219.0, cs = depth == 10 ? 896.0 : 224.0;
  const double k[3] = {kr, kg, kb}, off[3] = {depth == 10 ? 64.0 : 16.0, depth == 10 ? 512.0 : 128.0, depth == 10 ? 512.0 : 128.0};
  double a[3][3];
  for (int j = 0; j < 3; ++j) {
    a[0][j] = ys * k[j];
    a[1][j] = cs * (((j == 2 ? 1.0 : 0.0) - k[j]) / (2.0 * (1.0 - kb)));
    a[2][j] = cs * (((j == 0 ? 1.0 : 0.0) - k[j]) / (2.0 * (1.0 - kr)));
  }
  double cof[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      cof[i][j] = a[(i + 1) % 3][(j + 1) % 3] * a[(i + 2) % 3][(j + 2) % 3] - a[(i + 1) % 3][(j + 2) % 3] * a[(i + 2) % 3][(j + 1) % 3];
  const double det = a[0][0] * cof[0][0] + a[0][1] * cof[0][1] + a[0][2] * cof[0][2];
  for (int i = 0; i < 3; ++i) {
    double inv[3];
    for (int j = 0; j < 3; ++j) {
      inv[j] = cof[j][i] / det;
      yuv2rgb12[4 * i + j] = (float)inv[j];
      rgb2yuv12[4 * i + j] = (float)a[i][j];
    }
    yuv2rgb12[4 * i + 3] = (float)(-(inv[0] * off[0] + inv[1] * off[1] + inv[2] * off[2]));
    rgb2yuv12[4 * i + 3] = (float)off[i];
  }
}

extern "C" int vs_nv12_default_color(float* yuv2rgb12, float* rgb2yuv12) {
  VS_REQUIRE(yuv2rgb12 && rgb2yuv12);
  nv12_default_color(yuv2rgb12, rgb2yuv12);
  return VS_OK;
}

extern "C" int vs_yuv420_default_color(int depth, float* yuv2rgb12, float* rgb2yuv12) {
  VS_REQUIRE(yuv2rgb12 && rgb2yuv12 && (depth == 8 || depth == 10));
  yuv420_default_color(depth, yuv2rgb12, rgb2yuv12);
  return VS_OK;
}

extern "C" int vs_model_set_nv12_color(vs_model_t* m, const float* yuv2rgb12, const float* rgb2yuv12) {
  VS_REQUIRE(m && yuv2rgb12 && rgb2yuv12);
  std::memcpy(m->yuv2rgb12, yuv2rgb12, sizeof(m->yuv2rgb12));
  std::memcpy(m->rgb2yuv12, rgb2yuv12, sizeof(m->rgb2yuv12));
  return VS_OK;
}

extern "C" void vs_model_destroy(vs_model_t* m) {
  if (!m) return;
  for (void* d : m->dev) (void)hipFree(d);
  delete m;
}

extern "C" int64_t vs_model_workspace_bytes(const vs_model_t* m, int frames, int H, int W, int step) {
  if (!m || frames <= 0 || H <= 0 || W <= 0 || step < 1) return -1;
  Runner e{const_cast<vs_model_t*>(m), nullptr, 0, 0, nullptr};
  e.embed(nullptr, 0, nullptr, 1, frames, H, W, step, 0, 1, 1, nullptr, nullptr);
  Runner dt{const_cast<vs_model_t*>(m), nullptr, 0, 0, nullptr};
  dt.detect(nullptr, 0, frames, H, W, 1, nullptr);
  return std::max(e.used, dt.used) + 256;
}

// io_u8 = 2: uint8 NV12 [frames][3H/2][W], contiguous (pitch W), as a surface of the 4:2:0 path
static vs_yuv_surface_t any_surface(const vs_yuv420_surface_t& s) {          // the same surface with its chroma format named
  vs_yuv_surface_t r;
  static_assert(sizeof(r) == sizeof(s), "vs_yuv_surface_t is vs_yuv420_surface_t with `chroma` in the reserved member");
  std::memcpy(&r, &s, sizeof(r));
  r.chroma = 420;
  return r;
}
static vs_yuv_surface_t nv12_contiguous(const void* frames, int H, int W) { return any_surface(vs_nv12_surface(frames, H, W, (int64_t)W * (H / 2 * 3))); }

extern "C" int vs_model_embed(vs_model_t* m, const void* imgs, const int32_t* msgs, int n_msgs, int frames, int H, int W, int step,
                              int video_mode, int lowres_attenuation, int antialias, int io_u8, void* imgs_w, float* preds_w, void* ws,
                              int64_t ws_bytes, void* stream) {
  VS_REQUIRE(m && imgs && msgs && imgs_w && ws && frames > 0 && H > 0 && W > 0 && step >= 1 && ((uintptr_t)ws & 255) == 0);
  const int nk = (frames + step - 1) / step;
  VS_REQUIRE(n_msgs == 1 || n_msgs == nk);
  VS_REQUIRE(video_mode >= 0 && video_mode <= 2);
  Runner r{m, static_cast<char*>(ws), ws_bytes, 0, stream};
  if (io_u8) VS_REQUIRE(m->c.clamp);
  vs_yuv_surface_t in, out;
  if (io_u8 == 2) {       // the 4:2:0 path on two contiguous nv12 surfaces, with the model's stored colour
    VS_REQUIRE(!(H & 1) && !(W & 1));
    if (preds_w) return VS_ERR_UNSUPPORTED;
    in = nv12_contiguous(imgs, H, W);
    out = nv12_contiguous(imgs_w, H, W);
    r.ysrc = &in; r.ydst = &out; r.ydec = m->yuv2rgb12; r.yenc = m->rgb2yuv12;
    io_u8 = 3;
  }
  r.embed(imgs, io_u8, msgs, n_msgs, frames, H, W, step, video_mode, lowres_attenuation, antialias, imgs_w, preds_w);
  return r.rc;
}

extern "C" int64_t vs_model_embed_psnr_workspace_bytes(const vs_model_t* m, int frames, int H, int W, int step) {
  if (!m || frames <= 0 || H <= 0 || W <= 0 || step < 1) return -1;
  const Runner::Psnr p{42.f, 0, 0.f, nullptr};
  Runner e{const_cast<vs_model_t*>(m), nullptr, 0, 0, nullptr};
  e.psnr = &p;
  e.embed(nullptr, 0, nullptr, 1, frames, H, W, step, 0, 1, 1, nullptr, nullptr);
  return e.used + 256;
}

extern "C" int vs_model_embed_psnr(vs_model_t* m, const void* imgs, const int32_t* msgs, int n_msgs, int frames, int H, int W, int step,
                                   int video_mode, int lowres_attenuation, int antialias, int io_u8, float target_db, int per_clip,
                                   float max_scale, void* imgs_w, float* preds_w, float* scale_out, void* ws, int64_t ws_bytes,
                                   void* stream) {
  VS_REQUIRE(m && imgs && msgs && imgs_w && scale_out && ws && frames > 0 && H > 0 && W > 0 && step >= 1 && ((uintptr_t)ws & 255) == 0);
  VS_REQUIRE(std::isfinite(target_db));
  const int nk = (frames + step - 1) / step;
  VS_REQUIRE(n_msgs == 1 || n_msgs == nk);
  VS_REQUIRE(video_mode >= 0 && video_mode <= 2);
  if (io_u8 != 0 && io_u8 != 1) return VS_ERR_UNSUPPORTED;      // (the YUV and packed RGB routes keep the fixed strength)
  if (io_u8) VS_REQUIRE(m->c.clamp);
  const Runner::Psnr p{target_db, per_clip ? 1 : 0, max_scale, scale_out};
  Runner r{m, static_cast<char*>(ws), ws_bytes, 0, stream};
  r.psnr = &p;
  r.embed(imgs, io_u8, msgs, n_msgs, frames, H, W, step, video_mode, lowres_attenuation, antialias, imgs_w, preds_w);
  return r.rc;
}

extern "C" int vs_model_detect(vs_model_t* m, const void* imgs, int frames, int H, int W, int antialias, int io_u8, float* logits, void* ws,
                               int64_t ws_bytes, void* stream) {
  VS_REQUIRE(m && imgs && logits && ws && frames > 0 && H > 0 && W > 0 && ((uintptr_t)ws & 255) == 0);
  Runner r{m, static_cast<char*>(ws), ws_bytes, 0, stream};
  vs_yuv_surface_t in;
  if (io_u8 == 2) {
    VS_REQUIRE(!(H & 1) && !(W & 1));
    in = nv12_contiguous(imgs, H, W);
    r.ysrc = &in; r.ydec = m->yuv2rgb12;
    io_u8 = 3;
  }
  r.detect(imgs, io_u8, frames, H, W, antialias, logits);
  return r.rc;
}

static bool yuv420_format_known(const vs_yuv420_surface_t& s) {
  return (s.depth == 8 && !s.msb_aligned && (s.planar == 0 || s.planar == 1)) || (s.depth == 10 && s.planar == 0 && s.msb_aligned == 1) ||
         (s.depth == 10 && s.planar == 1 && !s.msb_aligned);
}

extern "C" int vs_model_embed_yuv420(vs_model_t* m, const vs_yuv420_surface_t* in, const vs_yuv420_surface_t* out, const float* yuv2rgb12,
                                     const float* rgb2yuv12, const int32_t* msgs, int n_msgs, int frames, int H, int W, int step,
                                     int video_mode, int lowres_attenuation, int antialias, void* ws, int64_t ws_bytes, void* stream) {
  VS_REQUIRE(m && in && out && msgs && ws && frames > 0 && H > 0 && W > 0 && step >= 1 && ((uintptr_t)ws & 255) == 0);
  VS_REQUIRE(!yuv2rgb12 == !rgb2yuv12);
  const int nk = (frames + step - 1) / step;
  VS_REQUIRE(n_msgs == 1 || n_msgs == nk);
  VS_REQUIRE(video_mode >= 0 && video_mode <= 2);
  VS_REQUIRE(m->c.clamp && !(H & 1) && !(W & 1));
  if (!yuv420_format_known(*in) || in->planar != out->planar || in->depth != out->depth || in->msb_aligned != out->msb_aligned)
    return VS_ERR_UNSUPPORTED;
  const vs_yuv_surface_t sin = any_surface(*in), sout = any_surface(*out);
  return vs_model_embed_yuv(m, &sin, &sout, yuv2rgb12, rgb2yuv12, msgs, n_msgs, frames, H, W, step, video_mode, lowres_attenuation, antialias, ws,
                            ws_bytes, stream);
}

extern "C" int vs_model_detect_yuv420(vs_model_t* m, const vs_yuv420_surface_t* in, const float* yuv2rgb12, int frames, int H, int W,
                                      int antialias, float* logits, void* ws, int64_t ws_bytes, void* stream) {
  VS_REQUIRE(m && in && logits && ws && frames > 0 && H > 0 && W > 0 && ((uintptr_t)ws & 255) == 0);
  VS_REQUIRE(!(H & 1) && !(W & 1));
  if (!yuv420_format_known(*in)) return VS_ERR_UNSUPPORTED;
  const vs_yuv_surface_t sin = any_surface(*in);
  return vs_model_detect_yuv(m, &sin, yuv2rgb12, frames, H, W, antialias, logits, ws, ws_bytes, stream);
}

// one of the ten formats (the rule of vs_resize_pre_yuv); hm, wm: the low bits of H and W that must be zero
static bool yuv_format_known(const vs_yuv_surface_t& s, int& hm, int& wm) {
  const vs_yuv420_surface_t t{{}, {}, {}, s.planar, s.depth, s.msb_aligned, 0};
  if (!yuv420_format_known(t)) return false;
  if (s.chroma == 420) { hm = 1; wm = 1; return true; }
  if (s.chroma == 422) { hm = 0; wm = 1; return true; }
  if (s.chroma == 444 && s.planar == 1) { hm = 0; wm = 0; return true; }
  return false;
}

extern "C" int vs_model_embed_yuv(vs_model_t* m, const vs_yuv_surface_t* in, const vs_yuv_surface_t* out, const float* yuv2rgb12,
                                  const float* rgb2yuv12, const int32_t* msgs, int n_msgs, int frames, int H, int W, int step, int video_mode,
                                  int lowres_attenuation, int antialias, void* ws, int64_t ws_bytes, void* stream) {
  VS_REQUIRE(m && in && out && msgs && ws && frames > 0 && H > 0 && W > 0 && step >= 1 && ((uintptr_t)ws & 255) == 0);
  VS_REQUIRE(!yuv2rgb12 == !rgb2yuv12);
  const int nk = (frames + step - 1) / step;
  VS_REQUIRE(n_msgs == 1 || n_msgs == nk);
  VS_REQUIRE(video_mode >= 0 && video_mode <= 2);
  int hm = 0, wm = 0;
  const bool known = yuv_format_known(*in, hm, wm);
  VS_REQUIRE(m->c.clamp && (!known || (!(H & hm) && !(W & wm))));
  if (!known || in->planar != out->planar || in->depth != out->depth || in->msb_aligned != out->msb_aligned || in->chroma != out->chroma)
    return VS_ERR_UNSUPPORTED;
  float dec[12], enc[12];
  if (!yuv2rgb12) yuv420_default_color(in->depth, dec, enc);
  Runner r{m, static_cast<char*>(ws), ws_bytes, 0, stream};
  r.ysrc = in; r.ydst = out;
  r.ydec = yuv2rgb12 ? yuv2rgb12 : dec;
  r.yenc = rgb2yuv12 ? rgb2yuv12 : enc;
  r.embed(nullptr, 3, msgs, n_msgs, frames, H, W, step, video_mode, lowres_attenuation, antialias, nullptr, nullptr);
  return r.rc;
}

extern "C" int vs_model_detect_yuv(vs_model_t* m, const vs_yuv_surface_t* in, const float* yuv2rgb12, int frames, int H, int W, int antialias,
                                   float* logits, void* ws, int64_t ws_bytes, void* stream) {
  VS_REQUIRE(m && in && logits && ws && frames > 0 && H > 0 && W > 0 && ((uintptr_t)ws & 255) == 0);
  int hm = 0, wm = 0;
  if (!yuv_format_known(*in, hm, wm)) return VS_ERR_UNSUPPORTED;
  VS_REQUIRE(!(H & hm) && !(W & wm));
  float dec[12], enc[12];
  if (!yuv2rgb12) yuv420_default_color(in->depth, dec, enc);
  Runner r{m, static_cast<char*>(ws), ws_bytes, 0, stream};
  r.ysrc = in;
  r.ydec = yuv2rgb12 ? yuv2rgb12 : dec;
  r.detect(nullptr, 3, frames, H, W, antialias, logits);
  return r.rc;
}

// ---- packed RGB surfaces (rgbpack.hip): the two entry points above with the surfaces of vs_resize_pre_rgb / vs_embed_tail_rgb
extern "C" int vs_model_embed_rgb(vs_model_t* m, const vs_rgb_surface_t* in, const vs_rgb_surface_t* out, const int32_t* msgs, int n_msgs,
                                  int frames, int H, int W, int step, int video_mode, int lowres_attenuation, int antialias, void* ws,
                                  int64_t ws_bytes, void* stream) {
  VS_REQUIRE(m && in && out && in->data && out->data && msgs && ws && frames > 0 && H > 0 && W > 0 && step >= 1 && ((uintptr_t)ws & 255) == 0);
  const int nk = (frames + step - 1) / step;
  VS_REQUIRE(n_msgs == 1 || n_msgs == nk);
  VS_REQUIRE(video_mode >= 0 && video_mode <= 2);
  VS_REQUIRE(m->c.clamp && in->data != out->data);
  if (in->format < VS_RGB_RGB24 || in->format > VS_RGB_X2BGR10 || in->format != out->format) return VS_ERR_UNSUPPORTED;
  Runner r{m, static_cast<char*>(ws), ws_bytes, 0, stream};
  r.psrc = in; r.pdst = out;
  r.embed(nullptr, 4, msgs, n_msgs, frames, H, W, step, video_mode, lowres_attenuation, antialias, nullptr, nullptr);
  return r.rc;
}

extern "C" int vs_model_detect_rgb(vs_model_t* m, const vs_rgb_surface_t* in, int frames, int H, int W, int antialias, float* logits, void* ws,
                                   int64_t ws_bytes, void* stream) {
  VS_REQUIRE(m && in && in->data && logits && ws && frames > 0 && H > 0 && W > 0 && ((uintptr_t)ws & 255) == 0);
  if (in->format < VS_RGB_RGB24 || in->format > VS_RGB_X2BGR10) return VS_ERR_UNSUPPORTED;
  Runner r{m, static_cast<char*>(ws), ws_bytes, 0, stream};
  r.psrc = in;
  r.detect(nullptr, 4, frames, H, W, antialias, logits);
  return r.rc;
}

// ---- half-precision surfaces (halfpix.hip, include/videoseal_half.h): the same two entry points on vs_half_surface_t.  The formats are
// checked by vs_resize_pre_half / vs_embed_tail_half; n_msgs = frames with step = 1 is image mode (a message per frame)
extern "C" int vs_model_embed_half(vs_model_t* m, const vs_half_surface_t* in, const vs_half_surface_t* out, const int32_t* msgs, int n_msgs,
                                   int frames, int H, int W, int step, int video_mode, int lowres_attenuation, int antialias, void* ws,
                                   int64_t ws_bytes, void* stream) {
  VS_REQUIRE(m && in && out && in->plane[0] && out->plane[0] && msgs && ws && frames > 0 && H > 0 && W > 0 && step >= 1 && ((uintptr_t)ws & 255) == 0);
  const int nk = (frames + step - 1) / step;
  VS_REQUIRE(n_msgs == 1 || n_msgs == nk);
  VS_REQUIRE(video_mode >= 0 && video_mode <= 2);
  VS_REQUIRE(m->c.clamp && in->plane[0] != out->plane[0]);
  if (in->elem != out->elem || in->layout != out->layout || in->components != out->components || in->value_range != out->value_range)
    return VS_ERR_UNSUPPORTED;
  Runner r{m, static_cast<char*>(ws), ws_bytes, 0, stream};
  r.hsrc = in; r.hdst = out;
  r.embed(nullptr, 5, msgs, n_msgs, frames, H, W, step, video_mode, lowres_attenuation, antialias, nullptr, nullptr);
  return r.rc;
}

extern "C" int vs_model_detect_half(vs_model_t* m, const vs_half_surface_t* in, int frames, int H, int W, int antialias, float* logits, void* ws,
                                    int64_t ws_bytes, void* stream) {
  VS_REQUIRE(m && in && in->plane[0] && logits && ws && frames > 0 && H > 0 && W > 0 && ((uintptr_t)ws & 255) == 0);
  Runner r{m, static_cast<char*>(ws), ws_bytes, 0, stream};
  r.hsrc = in;
  r.detect(nullptr, 5, frames, H, W, antialias, logits);
  return r.rc;
}
