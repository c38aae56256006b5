// Single-kernel C-ABI entry points (include/ddmi.h, "single-op entry points"): used by the GPU parity tests to check
// each kernel in isolation against a float64 restatement of the operation on the same inputs - a max-norm bar per
// tensor (test_ops_gpu.py, test_op_views_gpu.py, test_attn_views_gpu.py) and, for the f16x3 kernels, a per-element
// bound with a measured factor (test_f16x3_bound_gpu.py, test_vproj_tables_gpu.py) - with the operands inside
// poisoned guards where the entry takes views or row tables.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <utility>

#include "../../include/ddmi.h"
#include "common.h"
#include "decoder_mk.h"
#include "weights.h"
#include <vector>

namespace {
thread_local std::string g_op_err;
// dd_op_last_kernel: the configuration of the calling thread's last conv / GEMM launch (a dispatch that launched
// nothing leaves it)
thread_local const char* g_op_kernel = "";
thread_local const char* g_op_walk = "";
void ran(const ddmi::ConvRoute& r) {
  if (*r.config) g_op_walk = r.walk;
  if (*r.config) g_op_kernel = r.config;
}

template <class F>
int op_guard(F&& f) {
  try {
    f();
    return DD_OK;
  } catch (const std::invalid_argument& e) {
    g_op_err = e.what();
    return DD_ERR_INVALID;
  } catch (const std::exception& e) {
    g_op_err = e.what();
    return DD_ERR_RUNTIME;
  }
}
hipStream_t S(void* s) { return static_cast<hipStream_t>(s); }
}  // namespace

using namespace ddmi;

extern "C" {

const char* dd_op_last_error(void) { return g_op_err.c_str(); }

const char* dd_op_last_kernel(void) { return g_op_kernel; }

const char* dd_op_last_walk(void) { return g_op_walk; }

int dd_op_split_weights(const float* w, int rows, int K, uint16_t* hi, uint16_t* lo, uint16_t* b16, float* sinv,
                        int* ldh_out) {
  return op_guard([&] {
    if (!w || rows < 1 || K < 1) throw std::invalid_argument("dd_op_split_weights: null pointer or bad shape");
    Arena ar;  // host side only: never uploaded
    const SplitW x = prep_split(ar, w, rows, K);
    const size_t bytes = (size_t)rows * x.ldh * sizeof(uint16_t);
    if (hi) std::memcpy(hi, ar.host(x.hi), bytes);
    if (lo) std::memcpy(lo, ar.host(x.lo), bytes);
    if (b16) std::memcpy(b16, ar.host(x.b16), bytes);
    if (sinv) std::memcpy(sinv, ar.host(x.sinv), (size_t)rows * sizeof(float));
    if (ldh_out) *ldh_out = x.ldh;
  });
}

int dd_op_pack_mk_weights(const float* w, int nout, int nin, uint16_t* packed, float* sinv) {
  return op_guard([&] {
    if (!w || nout < 1 || nin < 1 || nin % 16 || nout % 32)
      throw std::invalid_argument("dd_op_pack_mk_weights: null pointer, nin % 16 or nout % 32");
    std::vector<_Float16> pk;
    std::vector<float> si;
    pack_mk_weights(w, nout, nin, pk, si);
    if (packed) std::memcpy(packed, pk.data(), pk.size() * sizeof(_Float16));
    if (sinv) std::memcpy(sinv, si.data(), si.size() * sizeof(float));
  });
}

int dd_op_mk_linear(const float* A, int K, const float* wgt, const float* bias, float* out, int N, void* stream) {
  return op_guard([&] {
    std::vector<float> hw((size_t)N * K);
    DD_HIP_CHECK(hipStreamSynchronize(S(stream)));
    DD_HIP_CHECK(hipMemcpy(hw.data(), wgt, hw.size() * sizeof(float), hipMemcpyDeviceToHost));
    std::vector<_Float16> pk;
    std::vector<float> sinv;
    pack_mk_weights(hw.data(), N, K, pk, sinv);
    Arena ar;
    const size_t wo = ar.add(reinterpret_cast<const float*>(pk.data()), pk.size() / 2);
    const size_t so = ar.add(sinv);
    ar.upload();
    MkLin m;
    m.w = reinterpret_cast<const uint4*>(ar.ptr(wo));
    m.s = ar.ptr(so);
    m.b = bias;
    m.nks = K / 16;
    launch_mk_linear_test(A, K, m, N, out, S(stream));
    DD_HIP_CHECK(hipStreamSynchronize(S(stream)));
  });
}

int dd_op_bevproj(const float* p3, int64_t p3_ld, const float* kvp, const float* wgt, const float* bias,
                  const float* ln_g, const float* ln_b, float* out, int B, int H, int W, int Hk, int Wk, void* stream) {
  return op_guard([&] {
    if (!bevproj_supported(256, 64, H, W, Hk, Wk)) throw std::invalid_argument("dd_op_bevproj: unsupported shape");
    std::vector<float> hw((size_t)256 * 64);
    DD_HIP_CHECK(hipStreamSynchronize(S(stream)));
    DD_HIP_CHECK(hipMemcpy(hw.data(), wgt, hw.size() * sizeof(float), hipMemcpyDeviceToHost));
    std::vector<_Float16> pk;
    std::vector<float> sinv;
    pack_mk_weights(hw.data(), 256, 64, pk, sinv);
    Arena ar;
    const size_t wo = ar.add(reinterpret_cast<const float*>(pk.data()), pk.size() / 2);
    const size_t so = ar.add(sinv);
    ar.upload();
    BevProjArgs a;
    a.p3 = p3;
    a.p3_ld = p3_ld;
    a.kvp = kvp;
    a.w = reinterpret_cast<const uint4*>(ar.ptr(wo));
    a.s = ar.ptr(so);
    a.bias = bias;
    a.g = ln_g;
    a.beta = ln_b;
    a.out = out;
    a.B = B;
    a.H = H;
    a.W = W;
    a.Hk = Hk;
    a.Wk = Wk;
    launch_bevproj(a, S(stream));
    DD_HIP_CHECK(hipStreamSynchronize(S(stream)));
  });
}

// the contiguous NHWC conv of dd_op_conv2d / dd_op_conv2d_x3 (the residual in the output's layout)
static ConvArgs conv2d_args(const float* in, int B, int H, int W, int Cin, const float* wgt, const float* bias,
                            const float* res, float* out, int Cout, int KH, int KW, int stride, int pad, int relu) {
  const int Ho = (H + 2 * pad - KH) / stride + 1, Wo = (W + 2 * pad - KW) / stride + 1;
  ConvArgs a = conv_args(nhwc(in, H, W, Cin), B, H, W, Cin, ConvGeom{KH, KW, stride, pad, Cout},
                         nhwc(out, Ho, Wo, Cout), relu, nhwc(res, Ho, Wo, Cout));
  a.wgt = wgt;
  a.bias = bias;
  return a;
}
// the split images of `x` (uploaded in `ar`) for prec 0 (f16x3) / 1 (bf16)
static void attach_split(ConvArgs& a, const Arena& ar, const SplitW& x, int prec, unsigned* flags) {
  a.prec = prec;
  a.wh = reinterpret_cast<const uint16_t*>(ar.ptr(prec ? x.b16 : x.hi));
  a.wl = reinterpret_cast<const uint16_t*>(ar.ptr(x.lo));
  a.wsinv = ar.ptr(x.sinv);
  a.ldh = x.ldh;
  a.flags = flags;
}

// The ops build the F(2,3) walk image (conv_x6) of every 3 x 3 / stride 1 / pad 1 conv with Cin % 32 == 0, whatever
// its size: DDMI_X6_WALK=2 then reaches the walk at test shapes.
static bool walk_geom(int KH, int KW, int stride, int pad, int Cin) {
  return KH == 3 && KW == 3 && stride == 1 && pad == 1 && Cin % 32 == 0;
}
static void attach_walk(ConvArgs& a, const Arena& ar, const SplitW& xw) {
  a.wh2 = reinterpret_cast<const uint16_t*>(ar.ptr(xw.hi));
  a.wl2 = reinterpret_cast<const uint16_t*>(ar.ptr(xw.lo));
  a.wsinv2 = ar.ptr(xw.sinv);
  a.ldh2 = xw.ldh;
}

int dd_op_conv2d(const float* in, int B, int H, int W, int Cin, const float* wgt, const float* bias, const float* res,
                 float* out, int Cout, int KH, int KW, int stride, int pad, int relu, void* stream) {
  return op_guard([&] {
    ran(launch_conv_gemm(conv2d_args(in, B, H, W, Cin, wgt, bias, res, out, Cout, KH, KW, stride, pad, relu),
                         S(stream)));
  });
}

int dd_op_conv2d_x3(const float* in, int B, int H, int W, int Cin, const float* wgt, const float* bias,
                    const float* res, float* out, int Cout, int KH, int KW, int stride, int pad, int relu, int prec,
                    unsigned* flags, void* stream) {
  return op_guard([&] {
    // split the (device) fp32 weights on the host exactly as dd_create does (weights.cpp:prep_split)
    const int K = KH * KW * Cin;
    std::vector<float> hw((size_t)Cout * K);
    DD_HIP_CHECK(hipStreamSynchronize(S(stream)));
    DD_HIP_CHECK(hipMemcpy(hw.data(), wgt, hw.size() * sizeof(float), hipMemcpyDeviceToHost));
    Arena ar;
    const SplitW x = prep_split(ar, hw.data(), Cout, K);
    const bool walk = prec == 0 && walk_geom(KH, KW, stride, pad, Cin);
    SplitW xw;
    if (walk) xw = prep_split_walk(ar, hw.data(), Cout, Cin);
    ar.upload();
    ConvArgs a = conv2d_args(in, B, H, W, Cin, wgt, bias, res, out, Cout, KH, KW, stride, pad, relu);
    if (prec != 0 && prec != 1) throw std::invalid_argument("prec must be 0 (f16x3) or 1 (bf16)");
    attach_split(a, ar, x, prec, flags);
    if (walk) attach_walk(a, ar, xw);
    // K-split scratch, as the forward provides it (runtime.cpp: run): small grids may take conv_x3's split form
    const int64_t mo = (int64_t)B * a.Ho * a.Wo * Cout;
    float* part = nullptr;
    if (prec == 0 && mo <= (1 << 20)) {
      DD_HIP_CHECK(hipMalloc(&part, (size_t)(8 * mo) * sizeof(float)));
      a.split_part = part;
      a.split_cap = 8 * mo;
    }
    ran(launch_conv_gemm(a, S(stream)));
    const hipError_t e = hipStreamSynchronize(S(stream));  // the split images die with `ar`
    if (part) DD_HIP_CHECK(hipFree(part));
    DD_HIP_CHECK(e);
  });
}

// u8: 0 = in is fp32, 1 = uint8 HWC, 2 = uint8 planar (lut: the bytes' 256 fp32 values)
static int dd_op_stem_pool_impl(const void* in, int src_c, int B, int H, int W, const float* wgt, const float* bias,
                                float* out, int prec, unsigned* flags, void* stream, int u8 = 0,
                                const float* lut = nullptr);

int dd_op_stem_pool_u8(const uint8_t* in, int layout, int B, int C, int H, int W, const float* lut, const float* wgt,
                       const float* bias, float* out, int prec, unsigned* flags, void* stream) {
  if (!in || !lut || (layout != 0 && layout != 1) || C < 1 || C > 3 || (layout == 0 && C != 3))
    return op_guard([&] {
      throw std::invalid_argument("stem_pool_u8: layout 0 (HWC, C = 3) or 1 (planar, C = 1..3), in and lut non-null");
    });
  return dd_op_stem_pool_impl(in, C, B, H, W, wgt, bias, out, prec, flags, stream, layout == 0 ? 1 : 2, lut);
}

int dd_op_stem_pool_x3(const float* in, int B, int H, int W, const float* wgt, const float* bias, float* out,
                       unsigned* flags, void* stream) {
  return dd_op_stem_pool(in, B, H, W, wgt, bias, out, 0, flags, stream);
}

int dd_op_stem_pool_nchw(const float* in, int B, int C, int H, int W, const float* wgt, const float* bias, float* out,
                         int prec, unsigned* flags, void* stream) {
  if (C < 1 || C > 3) return op_guard([&] { throw std::invalid_argument("stem_pool_nchw: C must be 1..3"); });
  return dd_op_stem_pool_impl(in, C, B, H, W, wgt, bias, out, prec, flags, stream);
}

int dd_op_stem_pool(const float* in, int B, int H, int W, const float* wgt, const float* bias, float* out, int prec,
                    unsigned* flags, void* stream) {
  return dd_op_stem_pool_impl(in, 0, B, H, W, wgt, bias, out, prec, flags, stream);
}

static int dd_op_stem_pool_impl(const void* in, int src_c, int B, int H, int W, const float* wgt, const float* bias,
                                float* out, int prec, unsigned* flags, void* stream, int u8, const float* lut) {
  return op_guard([&] {
    if (prec != 0 && prec != 1) throw std::invalid_argument("stem_pool: prec must be 0 (f16x3) or 1 (bf16)");
    const int Cin = 4, Cout = 64, K = 7 * 7 * Cin;
    std::vector<float> hw((size_t)Cout * K);
    DD_HIP_CHECK(hipStreamSynchronize(S(stream)));
    DD_HIP_CHECK(hipMemcpy(hw.data(), wgt, hw.size() * sizeof(float), hipMemcpyDeviceToHost));
    Arena ar;
    const SplitW x = prep_split(ar, hw.data(), Cout, K);
    ar.upload();
    // the kernel writes only the pooled map: no stem output view
    ConvArgs a = conv_args(nhwc(u8 ? nullptr : static_cast<const float*>(in), H, W, Cin), B, H, W, Cin,
                           ConvGeom{7, 7, 2, 3, Cout}, View4{}, true);
    a.wgt = wgt;
    a.bias = bias;
    attach_split(a, ar, x, prec, flags);
    const int hp = (a.Ho + 2 - 3) / 2 + 1, wp = (a.Wo + 2 - 3) / 2 + 1;
    // NCHW input of src_c channels: the kernel reads its address from a device word
    const void** word = nullptr;
    if (src_c) {
      DD_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&word), sizeof(const void*)));
      DD_HIP_CHECK(hipMemcpy(word, &in, sizeof(const void*), hipMemcpyHostToDevice));
    }
    bool ok = false;
    try {
      const ConvRoute r = launch_stem_pool(a, out, hp, wp, S(stream), src_c ? word : nullptr, src_c, u8, lut);
      ran(r);
      ok = r.kernel != nullptr;
      DD_HIP_CHECK(hipStreamSynchronize(S(stream)));  // the split images die with `ar`
    } catch (...) {
      if (word) (void)hipFree(word);
      throw;
    }
    if (word) DD_HIP_CHECK(hipFree(word));
    if (!ok) throw std::invalid_argument("stem_pool: shape not supported");
  });
}

int dd_build_camera(const uint8_t* cams, int B, int src_h, int src_w, float* out, int out_h, int out_w,
                    void* stream) {
  return op_guard([&] {
    if (!cams || !out) throw std::invalid_argument("null pointer");
    launch_camera_feature(cams, B, src_h, src_w, out, out_h, out_w, S(stream));
  });
}

int dd_build_lidar(const float* xyz, const int64_t* offsets, int B, int channels, float* out, int resolution,
                   float range_lo, float range_hi, int pixels_per_meter, float max_height, float split_height,
                   int hist_max, long long max_points, void* stream) {
  return op_guard([&] {
    if (!offsets || !out || (!xyz && max_points > 0)) throw std::invalid_argument("null pointer");
    launch_lidar_feature(xyz, offsets, B, channels, out, resolution, range_lo, range_hi, pixels_per_meter,
                         max_height, split_height, hist_max, max_points, S(stream));
  });
}

int dd_build_camera_u8(const uint8_t* cams, int B, int src_h, int src_w, uint8_t* out, int out_h, int out_w,
                       void* stream) {
  return op_guard([&] {
    if (!cams || !out) throw std::invalid_argument("null pointer");
    launch_camera_feature_u8(cams, B, src_h, src_w, out, out_h, out_w, S(stream));
  });
}

int dd_build_lidar_u8(const float* xyz, const int64_t* offsets, int B, int channels, uint8_t* out, int resolution,
                      float range_lo, float range_hi, int pixels_per_meter, float max_height, float split_height,
                      int hist_max, long long max_points, void* stream) {
  return op_guard([&] {
    if (!offsets || !out || (!xyz && max_points > 0)) throw std::invalid_argument("null pointer");
    launch_lidar_feature_u8(xyz, offsets, B, channels, out, resolution, range_lo, range_hi, pixels_per_meter,
                            max_height, split_height, hist_max, max_points, S(stream));
  });
}

int dd_op_gemm(const float* A, int M, int K, const float* W, const float* bias, const float* res, float* C, int N,
               int relu, void* stream) {
  return op_guard([&] {
    // M groups of one row each
    ConvArgs a = gemm_args(row_view(A, K, K), M, 1, K, N, row_view(C, N, N), relu, row_view(res, N, N));
    a.wgt = W;
    a.bias = bias;
    ran(launch_conv_gemm(a, S(stream)));
  });
}

int dd_op_gemm_batched(const float* A, const float* Bm, float* C, int batch, int M, int N, int K, int kn,
                       void* stream) {
  return op_guard([&] {
    ConvArgs a = gemm_args(row_view(A, K, K), M, 1, K, N, row_view(C, N, N));
    a.wgt = Bm;
    a.ldb = kn ? N : K;
    a.b_kn = kn;
    a.batch = batch;
    a.zdiv = 1;
    a.in_z1 = (int64_t)M * K;
    a.w_z1 = (int64_t)K * N;
    a.out_z1 = (int64_t)M * N;
    ran(launch_conv_gemm(a, S(stream)));
  });
}

int dd_op_layernorm(const float* x, const float* res, int res_div, const float* g, const float* b,
                    const float* film_scale, const float* film_shift, float* y, int rows, int C, void* stream) {
  return op_guard([&] {
    launch_layernorm(x, C, res, C, res_div, g, b, film_scale, film_shift, y, C, rows, C, S(stream));
  });
}

int dd_bev_semantic_loss(const float* logits, const unsigned char* target, int B, int C, int H, int W, float* work,
                         float* loss, void* stream) {
  return op_guard([&] {
    if (!logits || !target || !work || !loss || B < 1 || C < 1 || C > 255 || H < 1 || W < 1)
      throw std::invalid_argument("dd_bev_semantic_loss: null pointer or bad shape");
    launch_bev_ce(logits, target, work, loss, B, C, H * W, S(stream));
  });
}

size_t dd_bev_semantic_loss_work(int B, int H, int W) { return bev_ce_partials(B, H * W); }

int dd_op_softmax_rows(float* x, int rows, int L, float scale, void* stream) {
  return op_guard([&] { launch_softmax_rows(x, L, rows, L, scale, S(stream)); });
}

int dd_op_bilinear(const float* in, int B, int Hi, int Wi, int C, float* out, int Ho, int Wo, void* stream) {
  return op_guard([&] {
    View4 a{const_cast<float*>(in), (int64_t)Hi * Wi * C, (int64_t)Wi * C, C, 1};
    View4 o{out, (int64_t)Ho * Wo * C, (int64_t)Wo * C, C, 1};
    launch_bilinear(a, B, Hi, Wi, C, o, Ho, Wo, (float)Hi / (float)Ho, (float)Wi / (float)Wo, 0, S(stream));
  });
}

int dd_op_bilinear_add(const float* in, int B, int Hi, int Wi, int C, float* out, int Ho, int Wo, void* stream) {
  return op_guard([&] {
    View4 a{const_cast<float*>(in), (int64_t)Hi * Wi * C, (int64_t)Wi * C, C, 1};
    View4 o{out, (int64_t)Ho * Wo * C, (int64_t)Wo * C, C, 1};
    launch_bilinear(a, B, Hi, Wi, C, o, Ho, Wo, (float)Hi / (float)Ho, (float)Wi / (float)Wo, 1, S(stream));
  });
}

int dd_op_maxpool3x3s2(const float* in, int B, int H, int W, int C, float* out, void* stream) {
  return op_guard([&] {
    const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
    launch_maxpool3x3s2(in, out, B, H, W, C, Ho, Wo, S(stream));
  });
}

int dd_op_avgpool(const float* in, int B, int H, int W, int C, int oh, int ow, float* out, void* stream) {
  return op_guard([&] {
    View4 o{out, (int64_t)oh * ow * C, (int64_t)ow * C, C, 1};
    launch_avgpool(in, B, H, W, C, oh, ow, o, nullptr, S(stream));
  });
}

int dd_op_bev_sample_attn(const float* logits, const float* pts, const float* value, float* out, int B, int Q, int P,
                          int Hv, int Wv, int C, void* stream) {
  return op_guard([&] {
    launch_bev_sample_attn(logits, pts, value, out, B, Q, P, Hv, Wv, C, 1.0f / 32.0f, 1.0f / 32.0f, S(stream));
  });
}

int dd_op_mha_small(const float* q, const float* k, const float* v, float* out, int B, int Lq, int Lk, int nh, int hd,
                    void* stream) {
  return op_guard([&] {
    const int d = nh * hd;
    launch_mha_small(q, d, k, v, d, out, d, B, Lq, Lk, nh, hd, (int64_t)Lq * d, (int64_t)Lk * d, (int64_t)Lq * d,
                     S(stream));
  });
}

int dd_op_gpt_attention(const float* qkv, float* y, int B, int T, int C, int heads, int prec, void* stream) {
  return op_guard([&] { launch_gpt_attention(qkv, B, T, C, heads, y, prec, S(stream)); });
}

int dd_op_gpt_attention_rows(const float* qkv, float* y, int B, int T, int C, int heads, int prec, int q_first,
                             int q_count, int waves, void* stream) {
  return op_guard([&] {
    if (q_count < 1) throw std::invalid_argument("dd_op_gpt_attention_rows: q_count < 1");
    launch_gpt_attention(qkv, B, T, C, heads, y, prec, S(stream), q_first, q_count, waves);
  });
}

int dd_op_layernorm_groups(const float* x, const float* g, const float* b, float* y, int groups, int group_rows,
                           long long group_stride, int C, void* stream) {
  return op_guard([&] {
    if (groups < 1 || group_rows < 1 || group_stride < (long long)group_rows * C)
      throw std::invalid_argument("dd_op_layernorm_groups: groups, group_rows >= 1 and non-overlapping groups");
    launch_layernorm(x, C, nullptr, 0, 1, g, b, nullptr, nullptr, y, C, groups * group_rows, C, S(stream), 0, 0,
                     group_rows, group_stride);
  });
}

size_t dd_op_conv_desc_size(void) { return sizeof(dd_op_conv_desc); }

static View4 view_of(const dd_op_view& v) { return {v.p, v.sn, v.sh, v.sw, v.sc}; }

int dd_op_conv_view(dd_op_conv_desc* d, void* stream) {
  return op_guard([&] {
    if (!d) throw std::invalid_argument("dd_op_conv_view: null descriptor");
    d->fused_ln = d->fused_pool = 0;
    if (!d->in.p || !d->out.p || !d->wgt) throw std::invalid_argument("dd_op_conv_view: null in, out or wgt");
    if (d->mode < 0 || d->mode > 2) throw std::invalid_argument("dd_op_conv_view: mode must be 0, 1 or 2");
    if (d->N < 1 || d->H < 1 || d->W < 1 || d->Cin < 1 || d->Cout < 1 || d->KH < 1 || d->KW < 1 || d->stride < 1 ||
        d->pad < 0)
      throw std::invalid_argument("dd_op_conv_view: bad geometry");
    for (const dd_op_view* v : {&d->in, &d->out, &d->res, &d->pool_out, &d->pool_add})
      if (v->p && v->sc != 1) throw std::invalid_argument("dd_op_conv_view: the operands' channel stride is 1");
    const int64_t K = (int64_t)d->KH * d->KW * d->Cin;
    const bool sliced = d->k0 != 0 || d->ldb != K;
    if (sliced && (d->KH != 1 || d->KW != 1 || d->k0 < 0 || d->k0 % 8 || d->Cin % 8 || d->k0 + K > d->ldb))
      throw std::invalid_argument("dd_op_conv_view: a K slice needs a 1 x 1 geometry, k0 % 8 == 0, Cin % 8 == 0 and "
                                  "k0 + Cin <= ldb");
    const ConvGeom g{d->KH, d->KW, d->stride, d->pad, d->Cout};
    const bool rows = d->KH == 1 && d->KW == 1 && d->stride == 1 && d->pad == 0 && d->W == 1;
    ConvArgs a = rows ? gemm_args(view_of(d->in), d->N, d->H, d->Cin, d->Cout, view_of(d->out), d->relu,
                                  view_of(d->res))
                      : conv_args(view_of(d->in), d->N, d->H, d->W, d->Cin, g, view_of(d->out), d->relu,
                                  view_of(d->res));
    a.wgt = d->wgt;
    a.bias = d->bias;
    a.route_rows = d->route_rows;
    // modes 1 / 2: the whole weight (every K of its rows) split on the host exactly as dd_create does
    Arena ar;
    DD_HIP_CHECK(hipStreamSynchronize(S(stream)));
    if (d->mode) {
      std::vector<float> hw((size_t)d->Cout * d->ldb);
      DD_HIP_CHECK(hipMemcpy(hw.data(), d->wgt, hw.size() * sizeof(float), hipMemcpyDeviceToHost));
      const SplitW x = prep_split(ar, hw.data(), d->Cout, (int)d->ldb);
      const bool walk = d->mode == 1 && !sliced && walk_geom(d->KH, d->KW, d->stride, d->pad, d->Cin);
      SplitW xw;
      if (walk) xw = prep_split_walk(ar, hw.data(), d->Cout, d->Cin);
      ar.upload();
      attach_split(a, ar, x, d->mode - 1, d->flags);
      if (walk) attach_walk(a, ar, xw);
    }
    if (sliced) slice_k(a, d->k0, d->ldb);
    if (d->ln_out) fold_ln(a, d->ln_out, d->ln_g, d->ln_b);
    if (d->pool_out.p) pool_into(a, d->pool_p, view_of(d->pool_out), view_of(d->pool_add));
    // K-split scratch, as the forward provides it (runtime.cpp: run)
    const int64_t mo = (int64_t)a.Nimg * a.Ho * a.Wo * a.Cout;
    float* part = nullptr;
    if (d->mode == 1 && mo <= (1 << 20)) {
      DD_HIP_CHECK(hipMalloc(&part, (size_t)(8 * mo) * sizeof(float)));
      a.split_part = part;
      a.split_cap = 8 * mo;
    }
    hipError_t e = hipSuccess;
    try {
      const ConvRoute r = launch_conv_gemm(a, S(stream));
      ran(r);
      d->fused_ln = r.ln;
      d->fused_pool = r.pooled;
      e = hipStreamSynchronize(S(stream));  // the split images die with `ar`
    } catch (...) {
      if (part) (void)hipFree(part);
      throw;
    }
    if (part) DD_HIP_CHECK(hipFree(part));
    DD_HIP_CHECK(e);
  });
}

int dd_op_layernorm_ld(const float* x, int64_t ldx, const float* res, int64_t ldres, int res_div, const float* g,
                       const float* b, const float* film_scale, const float* film_shift, int film_div,
                       int64_t film_ld, float* y, int64_t ldy, int rows, int C, void* stream) {
  return op_guard([&] {
    if (!x || !y || !g || !b || rows < 0 || C < 1 || ldx < C || ldy < C)
      throw std::invalid_argument("dd_op_layernorm_ld: null pointer or a leading dimension below C");
    launch_layernorm(x, ldx, res, ldres, res_div, g, b, film_scale, film_shift, y, ldy, rows, C, S(stream), film_div,
                     film_ld);
  });
}

int dd_op_bilinear_view(const dd_op_view* in, int B, int Hi, int Wi, int C, const dd_op_view* out, int Ho, int Wo,
                        int accumulate, void* stream) {
  return op_guard([&] {
    if (!in || !out || !in->p || !out->p || B < 1 || Hi < 1 || Wi < 1 || C < 1 || Ho < 1 || Wo < 1)
      throw std::invalid_argument("dd_op_bilinear_view: null view or bad shape");
    launch_bilinear(view_of(*in), B, Hi, Wi, C, view_of(*out), Ho, Wo, (float)Hi / (float)Ho, (float)Wi / (float)Wo,
                    accumulate, S(stream));
  });
}

int dd_op_mha_small_view(const float* q, int64_t ldq, int64_t q_bstride, const float* k, const float* v, int64_t ldkv,
                         int64_t kv_bstride, float* out, int64_t ldo, int64_t o_bstride, int B, int Lq, int Lk, int nh,
                         int hd, int kv_div, void* stream) {
  return op_guard([&] {
    if (!q || !k || !v || !out) throw std::invalid_argument("dd_op_mha_small_view: null q, k, v or out");
    if (B < 1 || Lq < 1 || Lk < 1 || nh < 1 || hd < 1 || kv_div < 1)
      throw std::invalid_argument("dd_op_mha_small_view: B, Lq, Lk, nh, hd and kv_div must be positive");
    const int64_t d = (int64_t)nh * hd;
    if (ldq < d || ldkv < d || ldo < d)
      throw std::invalid_argument("dd_op_mha_small_view: a leading dimension below nh * hd");
    launch_mha_small(q, ldq, k, v, ldkv, out, ldo, B, Lq, Lk, nh, hd, q_bstride, kv_bstride, o_bstride, S(stream),
                     kv_div);
  });
}

int dd_op_bev_sample_attn_s(const float* logits, const float* pts, const float* value, float* out, int B, int Q, int P,
                            int Hv, int Wv, int C, int samples, float inv_max_x, float inv_max_y, void* stream) {
  return op_guard([&] {
    if (!logits || !pts || !value || !out)
      throw std::invalid_argument("dd_op_bev_sample_attn_s: null logits, pts, value or out");
    if (B < 1 || Q < 1 || P < 1 || Hv < 1 || Wv < 1 || C < 1 || samples < 1)
      throw std::invalid_argument("dd_op_bev_sample_attn_s: B, Q, P, Hv, Wv, C and samples must be positive");
    launch_bev_sample_attn(logits, pts, value, out, B, Q, P, Hv, Wv, C, inv_max_x, inv_max_y, S(stream), samples);
  });
}

int dd_op_bev_taps(const float* pts, int* rows, int* slots, int B, int Q, int P, int Hv, int Wv, float inv_max_x,
                   float inv_max_y, int samples, void* stream) {
  bool launched = true;
  const int rc = op_guard([&] {
    if (!pts || !rows) throw std::invalid_argument("dd_op_bev_taps: null pts or rows");
    if (B < 1 || Q < 1 || P < 1 || Hv < 1 || Wv < 1 || samples < 1)
      throw std::invalid_argument("dd_op_bev_taps: B, Q, P, Hv, Wv and samples must be positive");
    if (slots)
      launched = launch_bev_tap_dedup(pts, rows, slots, B, Q, P, Hv, Wv, inv_max_x, inv_max_y, S(stream), samples);
    else
      launch_bev_tap_rows(pts, rows, B, Q, P, Hv, Wv, inv_max_x, inv_max_y, S(stream), samples);
  });
  return rc != DD_OK ? rc : launched ? 1 : 0;
}

int dd_op_bev_sample_attn_gathered(const float* logits, const float* pts, const float* vrows, const int* slots,
                                   float* out, int B, int Q, int P, int Hv, int Wv, int C, float inv_max_x,
                                   float inv_max_y, void* stream) {
  return op_guard([&] {
    if (!logits || !pts || !vrows || !out)
      throw std::invalid_argument("dd_op_bev_sample_attn_gathered: null logits, pts, vrows or out");
    if (B < 1 || Q < 1 || P < 1 || Hv < 1 || Wv < 1 || C < 1)
      throw std::invalid_argument("dd_op_bev_sample_attn_gathered: B, Q, P, Hv, Wv and C must be positive");
    launch_bev_sample_attn_gathered(logits, pts, vrows, slots, out, B, Q, P, Hv, Wv, C, inv_max_x, inv_max_y,
                                    S(stream));
  });
}

int dd_op_vproj_limits(int* umax_rows, int* range_keys) {
  return op_guard([&] {
    if (!umax_rows || !range_keys) throw std::invalid_argument("dd_op_vproj_limits: null umax_rows or range_keys");
    vproj_limits(umax_rows, range_keys);
  });
}

namespace {
struct DevWords {  // a device scratch array, freed on every way out
  void* p = nullptr;
  void alloc(size_t bytes) { DD_HIP_CHECK(hipMalloc(&p, std::max<size_t>(bytes, 16))); }
  ~DevWords() {
    if (p) (void)hipFree(p);
  }
};
// a caller's row table, read back: counts within [0, cap] and every listed key a pixel of the map, so that neither
// kernel is launched on a table that would take it outside its operands
void vproj_check_table(const int* rows, const int* counts, int B, int cap, int nimg, const char* which) {
  std::vector<int> hc((size_t)B), hr((size_t)B * cap);
  DD_HIP_CHECK(hipMemcpy(hc.data(), counts, hc.size() * sizeof(int), hipMemcpyDeviceToHost));
  DD_HIP_CHECK(hipMemcpy(hr.data(), rows, hr.size() * sizeof(int), hipMemcpyDeviceToHost));
  for (int b = 0; b < B; ++b) {
    if (hc[b] < 0 || hc[b] > cap)
      throw std::invalid_argument(std::string("dd_op_vproj: ") + which + " counts outside [0, cap]");
    for (int l = 0; l < hc[b]; ++l) {
      const int k = hr[(size_t)b * cap + l];
      if (k < 0 || k >= nimg * 4096)
        throw std::invalid_argument(std::string("dd_op_vproj: ") + which + " rows name a pixel outside the map");
    }
  }
}
}  // namespace

int dd_op_vproj(const float* map, const float* wgt, const float* bias, const int* rows, const int* counts, float* out,
                int B, int cap, int nimg, int union_stage, int usplit, int umax, int ldh_pad, unsigned part_fill,
                unsigned* flags, const int* rows2, const int* counts2, float* out2, unsigned* fb_seen,
                unsigned* fb_after, unsigned* ucnt_after, void* stream) {
  return op_guard([&] {
    const std::pair<const void*, const char*> must[] = {{map, "map"},   {wgt, "wgt"},       {bias, "bias"},
                                                        {rows, "rows"}, {counts, "counts"}, {out, "out"}};
    for (const auto& m : must)
      if (!m.first) throw std::invalid_argument(std::string("dd_op_vproj: null ") + m.second);
    if (B < 1 || cap < 1 || (int64_t)B * cap > (1 << 22))
      throw std::invalid_argument("dd_op_vproj: B and cap must be positive, B * cap at most 2^22 rows");
    if (nimg < 0 || nimg > (1 << 16)) throw std::invalid_argument("dd_op_vproj: nimg must be 0 (B) .. 65536");
    if (union_stage != 0 && union_stage != 1) throw std::invalid_argument("dd_op_vproj: union_stage must be 0 or 1");
    if (ldh_pad < 0 || ldh_pad % 8 || ldh_pad > 1024)
      throw std::invalid_argument("dd_op_vproj: ldh_pad must be a multiple of 8 in 0 .. 1024");
    if ((rows2 != nullptr) != (counts2 != nullptr) || (rows2 != nullptr) != (out2 != nullptr))
      throw std::invalid_argument("dd_op_vproj: rows2, counts2 and out2 go together");
    constexpr int kCout = 256, kK = 9 * 256;
    const hipStream_t st = S(stream);
    DD_HIP_CHECK(hipStreamSynchronize(st));
    // split the (device) fp32 weights on the host exactly as dd_create does (weights.cpp:prep_split)
    std::vector<float> hw((size_t)kCout * kK);
    DD_HIP_CHECK(hipMemcpy(hw.data(), wgt, hw.size() * sizeof(float), hipMemcpyDeviceToHost));
    Arena ar;
    const SplitW x = prep_split(ar, hw.data(), kCout, kK);
    size_t hi = x.hi, lo = x.lo;
    const int ldh = x.ldh + ldh_pad;
    if (ldh_pad) {
      // the same images with longer rows; the padding holds fp16 NaNs, which neither kernel may read
      auto widen = [&](size_t off) {
        std::vector<uint16_t> img((size_t)kCout * ldh, (uint16_t)0x7e00);
        const uint16_t* src = reinterpret_cast<const uint16_t*>(ar.host(off));
        for (int r = 0; r < kCout; ++r)
          std::memcpy(&img[(size_t)r * ldh], src + (size_t)r * x.ldh, (size_t)x.ldh * sizeof(uint16_t));
        return ar.add(reinterpret_cast<const float*>(img.data()), img.size() / 2);
      };
      hi = widen(x.hi);
      lo = widen(x.lo);
    }
    ar.upload();
    const int nreal = nimg > 0 ? nimg : B;
    if (B <= 256 && nreal <= B) {  // (launch_vproj refuses the others before it launches anything)
      vproj_check_table(rows, counts, B, cap, nreal, "the first table's");
      if (rows2) vproj_check_table(rows2, counts2, B, cap, nreal, "the second table's");
    }
    // scratch as the forward holds it: zeroed fallback flags and arrival counters, partials of any content
    const size_t tiles = vproj_tiles(B, cap), words = 2 * ((tiles + 7) / 8 * 8);
    DevWords fb, ucnt, part;
    fb.alloc(words * sizeof(unsigned));
    ucnt.alloc(words * sizeof(unsigned));
    DD_HIP_CHECK(hipMemsetAsync(fb.p, 0, words * sizeof(unsigned), st));
    DD_HIP_CHECK(hipMemsetAsync(ucnt.p, 0, words * sizeof(unsigned), st));
    if (union_stage && usplit > 1 && usplit <= 64) {
      const size_t n = (size_t)usplit * B * cap * kCout;
      part.alloc(n * sizeof(float));
      DD_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(part.p), (int)part_fill, n, st));
    }
    VprojArgs v;
    v.map = map;
    v.wh = reinterpret_cast<const uint16_t*>(ar.ptr(hi));
    v.wl = reinterpret_cast<const uint16_t*>(ar.ptr(lo));
    v.wsinv = ar.ptr(x.sinv);
    v.ldh = ldh;
    v.bias = bias;
    v.rows = rows;
    v.counts = counts;
    v.B = B;
    v.cap = cap;
    v.nimg = nimg;
    v.out = out;
    v.flags = flags;
    v.union_stage = union_stage;
    v.umax = umax;
    v.usplit = usplit;
    v.fb = static_cast<unsigned*>(fb.p);
    v.ucnt = static_cast<unsigned*>(ucnt.p);
    v.part = static_cast<float*>(part.p);
    if (fb_seen) std::memset(fb_seen, 0, 2 * tiles * sizeof(unsigned));
    try {  // (the split images die with `ar`, the scratch with this scope: the stream is drained on every way out)
      if (union_stage) {
        // the union launch, the flags it raised, then the gathered launch that computes those tiles and clears them
        launch_vproj(v, st, kVprojUnion);
        DD_HIP_CHECK(hipStreamSynchronize(st));
        if (fb_seen) DD_HIP_CHECK(hipMemcpy(fb_seen, fb.p, 2 * tiles * sizeof(unsigned), hipMemcpyDeviceToHost));
        launch_vproj(v, st, kVprojFallback);
      } else {
        launch_vproj(v, st);
      }
      if (rows2) {  // the second table on the scratch the first launch left, as one forward's layers follow each other
        v.rows = rows2;
        v.counts = counts2;
        v.out = out2;
        launch_vproj(v, st);
      }
    } catch (...) {
      (void)hipStreamSynchronize(st);
      throw;
    }
    DD_HIP_CHECK(hipStreamSynchronize(st));
    if (fb_after) DD_HIP_CHECK(hipMemcpy(fb_after, fb.p, 2 * tiles * sizeof(unsigned), hipMemcpyDeviceToHost));
    if (ucnt_after) DD_HIP_CHECK(hipMemcpy(ucnt_after, ucnt.p, 2 * tiles * sizeof(unsigned), hipMemcpyDeviceToHost));
  });
}

int dd_op_avgpool_view(const float* in, int B, int H, int W, int C, int oh, int ow, const dd_op_view* out,
                       const float* add, void* stream) {
  return op_guard([&] {
    if (!in || !out || !out->p) throw std::invalid_argument("dd_op_avgpool_view: null in or out view");
    if (B < 1 || H < 1 || W < 1 || C < 1 || oh < 1 || ow < 1)
      throw std::invalid_argument("dd_op_avgpool_view: B, H, W, C, oh and ow must be positive");
    launch_avgpool(in, B, H, W, C, oh, ow, view_of(*out), add, S(stream));
  });
}

}  // extern "C"
