// Keras DepthwiseConv2D with float, binary, quantized or ternary weights (include/qnn_abi_depthwise.h) on float32
// tensors and on packed codes.  Output channel c * M + m reads input channel c only, so there is no reduction over
// channels and nothing for the matrix pipe: a streaming kernel in the manner of qnn_pool.hip, with the integer
// arithmetic of the conv kernels and the shared float32 chain (qnn_epi_value / qnn_epi_code, qnn_common.h) behind it.
//
// k_dw_plain -- any window, dilation, depth_multiplier and store; 32-bit (float32 input: float64) sums.  qnn_pool.hip's lane
// map: one lane owns V consecutive 32-bit words (float32 output: V consecutive channels) of ONE output pixel, consecutive
// lanes own the next groups of that pixel and then of the next pixel.  V = 4 (16 bytes per lane) where the words per pixel
// divide by 4 and both pointers are 16-byte aligned, V = 1 otherwise.  It is the correctness form: per output channel and
// tap it loads one input word and one weight code again (an input word is re-read once per channel it holds).
//
// k_dw_pk16 -- depth_multiplier 1, 3x3, stride 1, no dilation, I4 / I8 codes in and out.  One lane owns one word of one
// output column and walks kRows output rows down it, its 9 x NP weight pairs and per-channel constants held in registers
// (loaded once per lane, not per tap or pixel); consecutive lanes own the next words, then the next column, so a wave reads
// runs of whole pixels.  A loaded word is unpacked once into 16-bit lane pairs -- nibbles (j, j + 4), bytes (j, j + 2): the
// two halves of the word shifted alike, so a pair costs one or two packed shifts -- and serves the three output rows it
// is a tap of: one packed multiply-add per two channels.  Exact while 9 * 2^(x_bits-1) * 2^wshift < 2^15 (pk16_ok).
//
// Index arithmetic in 32 bits by multiply-high (the entry refuses 2^31 output words), tensor offsets in 64 bits.  Taps
// outside the image are not loaded.
#include <new>

#include "qnn_sideconv.h"
#include "qnn_abi_depthwise.h"

struct qnn_dw_weights : SideWeights {      // d_wq, d_wcode: [kh*kw][cout], Keras' (kh, kw, C, M) order
    int kh, kw, C, M, cout;
    int stride, same_pad, dil_h, dil_w;
    uint32_t* d_wpk;         // [9][xcw][pairs per word] 16-bit code pairs in k_dw_pk16's order, or nullptr
};

namespace {

constexpr int kBlock = 256;

// ---- weights ----------------------------------------------------------------------------------------------------------
// 16-bit code pairs: word (t, w, p) = code of channel w*PW + p (low half) and of channel w*PW + p + PW/2 (high half)
__global__ __launch_bounds__(kBlock) void k_dw_pairs(const int32_t* __restrict__ wcode, uint32_t* __restrict__ wpk, int C,
                                                     int xcw, int pw) {
    const int np = pw / 2, total = 9 * xcw * np;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= total) return;
    const int p = i % np, w = (i / np) % xcw, t = i / (np * xcw);
    const int c0 = w * pw + p, c1 = c0 + np;
    const int lo = c0 < C ? wcode[t * C + c0] : 0, hi = c1 < C ? wcode[t * C + c1] : 0;
    wpk[i] = ((uint32_t)lo & 0xFFFFu) | ((uint32_t)hi << 16);
}

// ---- geometry ---------------------------------------------------------------------------------------------------------
struct DwGeom {
    int H, W, Ho, Wo, C, M, cout;
    int kh, kw, stride, pt, pl, dil_h, dil_w;
    int xcw;                   // words (float32: channels) per input pixel
    int ocw;                   // words (float32: channels) per output pixel
    int groups;                // items per output pixel = ocw / V
    FastDiv fd_g, fd_wo, fd_ho, fd_m;
};

struct Item {
    uint32_t q;                // output pixel (n, oy, ox) flattened
    int g, n, y0, x0;          // word group; image; the window's first row and column (may lie outside the image)
};

__device__ __forceinline__ Item decode(uint32_t i, const DwGeom& p) {
    Item it;
    it.q = qnn_div(i, p.fd_g);
    it.g = (int)(i - it.q * (uint32_t)p.groups);
    const uint32_t t = qnn_div(it.q, p.fd_wo);
    const int ox = (int)(it.q - t * (uint32_t)p.Wo);
    it.n = (int)qnn_div(t, p.fd_ho);
    const int oy = (int)(t - (uint32_t)it.n * (uint32_t)p.Ho);
    it.y0 = oy * p.stride - p.pt;
    it.x0 = ox * p.stride - p.pl;
    return it;
}

// the code of channel c of the packed pixel at `px`
template <int XS>
__device__ __forceinline__ int load_code(const uint32_t* __restrict__ px, int c) {
    if constexpr (XS == QNN_STORE_BIN) {
        return (int)((px[c >> 5] >> (c & 31)) & 1u) * 2 - 1;
    } else if constexpr (XS == QNN_STORE_T2) {
        const uint32_t mask = px[2 * (c >> 5)], sign = px[2 * (c >> 5) + 1];
        const int nz = (int)((mask >> (c & 31)) & 1u), pos = (int)((sign >> (c & 31)) & 1u);
        return nz * (2 * pos - 1);
    } else if constexpr (XS == QNN_STORE_I4) {
        return (int)(px[c >> 3] << (28 - 4 * (c & 7))) >> 28;
    } else {
        return (int)(px[c >> 2] << (24 - 8 * (c & 3))) >> 24;
    }
}

// ---- the plain form ---------------------------------------------------------------------------------------------------
// XS: the input's store.  The output's store is e.out_store (wave-uniform).  A lane walks its V output words, the
// channels of a word and the taps of a channel; a channel beyond cout - 1 is left out, so its bits stay zero.
template <int XS, int V>
__global__ __launch_bounds__(kBlock) void k_dw_plain(const void* __restrict__ x, const float* __restrict__ wq,
                                                     const int32_t* __restrict__ wcode, void* __restrict__ y,
                                                     const DwGeom p, const EpiArgs e, const uint32_t total) {
    const uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (i >= total) return;
    const Item it = decode(i, p);
    const int w0 = it.g * V;
    const int opw = qnn_per_word(e.out_store), obits = 32 / opw;
    const uint32_t omask = obits == 32 ? 0xFFFFFFFFu : (1u << obits) - 1u;
    uint32_t out[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        uint32_t word = 0;
        for (int j = 0; j < opw; ++j) {
            const int oc = (w0 + v) * opw + j;
            if (oc >= p.cout) break;
            const int c = (int)qnn_div((uint32_t)oc, p.fd_m);
            float val;
            if constexpr (XS == QNN_STORE_F32) {
                double acc = 0.0;
                for (int ky = 0; ky < p.kh; ++ky) {
                    const int yy = it.y0 + ky * p.dil_h;
                    if ((unsigned)yy >= (unsigned)p.H) continue;
                    for (int kx = 0; kx < p.kw; ++kx) {
                        const int xx = it.x0 + kx * p.dil_w;
                        if ((unsigned)xx >= (unsigned)p.W) continue;
                        const float a = ((const float*)x)[(((size_t)it.n * p.H + yy) * p.W + xx) * p.xcw + c];
                        acc += (double)a * (double)wq[(ky * p.kw + kx) * p.cout + oc];
                    }
                }
                val = (float)acc;
            } else {
                int acc = 0;
                for (int ky = 0; ky < p.kh; ++ky) {
                    const int yy = it.y0 + ky * p.dil_h;
                    if ((unsigned)yy >= (unsigned)p.H) continue;
                    for (int kx = 0; kx < p.kw; ++kx) {
                        const int xx = it.x0 + kx * p.dil_w;
                        if ((unsigned)xx >= (unsigned)p.W) continue;
                        const uint32_t* px = (const uint32_t*)x + (((size_t)it.n * p.H + yy) * p.W + xx) * p.xcw;
                        acc += load_code<XS>(px, c) * wcode[(ky * p.kw + kx) * p.cout + oc];
                    }
                }
                val = __fmul_rn((float)acc, e.scale);
            }
            val = qnn_epi_value(val, oc, e);
            if (e.out_store == QNN_STORE_F32) word = __float_as_uint(act_value(val, e));
            else word |= ((uint32_t)qnn_epi_code(val, e) & omask) << (j * obits);
        }
        out[v] = word;
    }
    store_words<V>((uint32_t*)y + (size_t)it.q * p.ocw + w0, out);
}

// ---- the 16-bit-lane form -----------------------------------------------------------------------------------------------
typedef short v2s __attribute__((ext_vector_type(2)));

template <int XS> struct Lay {
    static constexpr int PW = XS == QNN_STORE_I4 ? 8 : 4;
    static constexpr int BITS = 32 / PW;
    static constexpr int NP = PW / 2;      // 16-bit pairs per word
};

// pair k of a word: field k in the low half, field k + NP in the high half, both sign-extended
template <int BITS>
__device__ __forceinline__ v2s pair_of(uint32_t w, int k) {
    v2s h;
    __builtin_memcpy(&h, &w, 4);
    const short up = (short)(16 - BITS - k * BITS), down = (short)(16 - BITS);
    return (v2s)(h << up) >> down;
}

constexpr int kRows = 4;                   // output rows a lane walks

// One lane owns ONE word (PW channels) of one output column and walks kRows output rows down it; consecutive lanes own the
// next words of the pixel, then the next column, so every load instruction of a wave still reads a run of whole pixels.
// The lane's 9 x NP weight pairs and its channels' bias / BN constants are loaded ONCE, before the walk, and stay in
// registers.  Input row r of the kRows + 2 the walk touches is loaded as its three column words, each unpacked once and used
// by the (up to) three output rows r - ky it is a tap of.  A tap outside the image is read as the zero word (code 0 adds
// nothing).  FN is a template argument: the activation is chosen at compile time.  3x3, stride 1.
template <int XS, int FN>
__global__ __launch_bounds__(kBlock) void k_dw_pk16(const uint32_t* __restrict__ x, const uint32_t* __restrict__ wpk,
                                                    uint32_t* __restrict__ y, const DwGeom p, const EpiArgs e,
                                                    const uint32_t total) {
    constexpr int PW = Lay<XS>::PW, BITS = Lay<XS>::BITS, NP = Lay<XS>::NP;
    const uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (i >= total) return;
    // item -> (n, row block, ox, word); fd_g divides by the words per pixel, fd_ho by the row blocks per image
    const uint32_t q = qnn_div(i, p.fd_g);
    const int g = (int)(i - q * (uint32_t)p.groups);
    const uint32_t t = qnn_div(q, p.fd_wo);
    const int ox = (int)(q - t * (uint32_t)p.Wo);
    const int n = (int)qnn_div(t, p.fd_ho);
    const int oyb = ((int)t - n * (int)p.fd_ho.d) * kRows;

    v2s w[9][NP];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const uint32_t* wt = wpk + ((size_t)tap * p.xcw + g) * NP;
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const uint32_t wv = wt[k];
            __builtin_memcpy(&w[tap][k], &wv, 4);
        }
    }
    // the channels' constants, indexed by the field j of the word; the chain itself is qnn_epi_value / qnn_epi_code
    float cb[PW], ci[PW], cs[PW];
#pragma unroll
    for (int j = 0; j < PW; ++j) {
        const int c = min(g * PW + j, p.C - 1);
        cb[j] = e.bias ? e.bias[c] : 0.0f;
        ci[j] = e.bn_inv ? e.bn_inv[c] : 1.0f;
        cs[j] = e.bn_inv ? e.bn_shift[c] : 0.0f;
    }
    EpiArgs le = e;
    le.fn = FN;
    le.out_store = XS;
    le.trick_s = 0.0f;
    le.bias = e.bias ? cb : nullptr;
    le.bn_inv = e.bn_inv ? ci : nullptr;
    le.bn_shift = cs;

    v2s acc[kRows][NP];
#pragma unroll
    for (int o = 0; o < kRows; ++o)
#pragma unroll
        for (int k = 0; k < NP; ++k) acc[o][k] = (v2s)(0);
    const int x0 = ox - p.pl;
#pragma unroll
    for (int r = 0; r < kRows + 2; ++r) {
        const int iy = oyb - p.pt + r;
        const bool rowok = (unsigned)iy < (unsigned)p.H;
        const uint32_t* row = x + ((size_t)n * p.H + (rowok ? iy : 0)) * p.W * p.xcw + g;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = x0 + kx;
            const bool ok = rowok && (unsigned)ix < (unsigned)p.W;
            const uint32_t a = ok ? row[(size_t)ix * p.xcw] : 0u;
            v2s u[NP];
#pragma unroll
            for (int k = 0; k < NP; ++k) u[k] = pair_of<BITS>(a, k);
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int o = r - ky;              // compile time: the output row this input row is tap ky of
                if (o >= 0 && o < kRows) {
#pragma unroll
                    for (int k = 0; k < NP; ++k) acc[o][k] += u[k] * w[ky * 3 + kx][k];
                }
            }
        }
    }
    constexpr uint32_t MASK = (1u << BITS) - 1u;
#pragma unroll
    for (int o = 0; o < kRows; ++o) {
        const int oy = oyb + o;
        if (oy >= p.Ho) break;
        uint32_t word = 0;
#pragma unroll
        for (int k = 0; k < NP; ++k) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int j = k + h * NP;
                const int s = h ? (int)acc[o][k].y : (int)acc[o][k].x;
                const float val = qnn_epi_value(__fmul_rn((float)s, e.scale), j, le);
                const uint32_t code = (uint32_t)qnn_epi_code(val, le) & MASK;
                word |= (g * PW + j < p.C ? code : 0u) << (j * BITS);
            }
        }
        y[(((size_t)n * p.Ho + oy) * p.Wo + ox) * p.ocw + g] = word;
    }
}

bool pk16_ok(const qnn_dw_weights* w, int x_bits) {
    if (w->M != 1 || w->kh != 3 || w->kw != 3 || w->dil_h != 1 || w->dil_w != 1 || w->stride != 1 || !w->d_wpk) return false;
    if (x_bits < 1 || x_bits > w->store) return false;
    return (long)w->kh * w->kw * (1L << (x_bits - 1)) * (1L << w->wshift) < (1L << 15);
}

template <int XS>
void launch_plain(bool v4, const void* x, const qnn_dw_weights* w, void* y, const DwGeom& g, const EpiArgs& e,
                  uint32_t total, hipStream_t s) {
    const dim3 grid((total + kBlock - 1) / kBlock), block(kBlock);
    if (v4) hipLaunchKernelGGL((k_dw_plain<XS, 4>), grid, block, 0, s, x, w->d_wq, w->d_wcode, y, g, e, total);
    else hipLaunchKernelGGL((k_dw_plain<XS, 1>), grid, block, 0, s, x, w->d_wq, w->d_wcode, y, g, e, total);
}

template <int XS>
void launch_pk16(int fn, const void* x, const qnn_dw_weights* w, void* y, const DwGeom& g, const EpiArgs& e, uint32_t total,
                 hipStream_t s) {
    const dim3 grid((total + kBlock - 1) / kBlock), block(kBlock);
    const uint32_t* xu = (const uint32_t*)x;
    uint32_t* yu = (uint32_t*)y;
#define DW_PK16(F) hipLaunchKernelGGL((k_dw_pk16<XS, F>), grid, block, 0, s, xu, w->d_wpk, yu, g, e, total)
    if (fn == QNN_FN_BINARY_TANH) DW_PK16(QNN_FN_BINARY_TANH);
    else if (fn == QNN_FN_QUANTIZED_RELU) DW_PK16(QNN_FN_QUANTIZED_RELU);
    else if (fn == QNN_FN_QUANTIZED_LEAKYRELU) DW_PK16(QNN_FN_QUANTIZED_LEAKYRELU);
    else DW_PK16(QNN_FN_QUANTIZED_TANH);
#undef DW_PK16
}

void out_hw(const qnn_dw_weights* w, int H, int W, DwGeom* g) {
    qnn_same_pad_dilated(H, w->kh, w->stride, w->dil_h, w->same_pad, &g->Ho, &g->pt);
    qnn_same_pad_dilated(W, w->kw, w->stride, w->dil_w, w->same_pad, &g->Wo, &g->pl);
}

// prepack: the operand image of k_dw_pk16, where the shape can take that form
int pack_pairs(qnn_dw_weights* w, hipStream_t s) {
    if ((w->store != QNN_STORE_I4 && w->store != QNN_STORE_I8) || w->M != 1 || w->kh != 3 || w->kw != 3 || w->dil_h != 1 ||
        w->dil_w != 1)
        return QNN_OK;
    const int pw = qnn_per_word(w->store), pairs = 9 * w->xcw * (pw / 2);
    QNN_SIDE_HIP(hipMalloc(&w->d_wpk, (size_t)pairs * sizeof(uint32_t)));
    hipLaunchKernelGGL(k_dw_pairs, dim3((pairs + kBlock - 1) / kBlock), dim3(kBlock), 0, s, w->d_wcode, w->d_wpk, w->C, w->xcw,
                       pw);
    return QNN_OK;
}

}  // namespace

extern "C" int qnn_depthwise_prepack(int wkind, int wbits, float H, const float* kernel, int kh, int kw, int C,
                                     int depth_multiplier, const float* bias, int stride, int same_pad, int dil_h,
                                     int dil_w, int store, void* stream, qnn_dw_weights_t** out) {
    const char* who = "qnn_depthwise_prepack";
    const int M = depth_multiplier;
    QNN_REQUIRE(kernel && out, QNN_EINVAL, "%s: null pointer", who);
    QNN_REQUIRE(dil_h >= 1 && dil_w >= 1, QNN_EINVAL, "%s: dilation %d x %d (must be >= 1)", who, dil_h, dil_w);
    QNN_REQUIRE(dil_h <= QNN_MAX_DILATION && dil_w <= QNN_MAX_DILATION, QNN_EUNSUPPORTED,
                "%s: dilation %d x %d above QNN_MAX_DILATION = %d", who, dil_h, dil_w, QNN_MAX_DILATION);
    QNN_REQUIRE(stride >= 1, QNN_EINVAL, "%s: stride=%d", who, stride);
    QNN_REQUIRE(stride <= 2, QNN_EUNSUPPORTED, "%s: stride=%d (1 or 2)", who, stride);
    QNN_REQUIRE((dil_h == 1 && dil_w == 1) || stride == 1, QNN_EUNSUPPORTED,
                "%s: dilation %d x %d together with stride %d is not supported (dilation != 1 needs stride 1)", who, dil_h,
                dil_w, stride);
    QNN_REQUIRE(kh > 0 && kw > 0 && C > 0 && M > 0, QNN_EINVAL, "%s: kernel shape (%d,%d,%d,%d)", who, kh, kw, C, M);
    QNN_REQUIRE(kh <= QNN_DW_MAX_WINDOW && kw <= QNN_DW_MAX_WINDOW, QNN_EUNSUPPORTED,
                "%s: kernel %dx%d larger than %dx%d is not supported", who, kh, kw, QNN_DW_MAX_WINDOW, QNN_DW_MAX_WINDOW);
    QNN_REQUIRE((double)C * M * kh * kw < 1.0e9, QNN_EUNSUPPORTED, "%s: %d x %d channels", who, C, M);
    SideWeights common{};
    int rc = qnn_side_weights_check(who, wkind, wbits, H, store, &common);
    if (rc != QNN_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    qnn_dw_weights* w = new (std::nothrow) qnn_dw_weights();
    QNN_REQUIRE(w, QNN_ENOMEM, "%s: host allocation failed", who);
    *static_cast<SideWeights*>(w) = common;
    w->kh = kh; w->kw = kw; w->C = C; w->M = M; w->cout = C * M;
    w->stride = stride; w->same_pad = same_pad ? 1 : 0;
    w->dil_h = dil_h; w->dil_w = dil_w;
    w->xcw = store == QNN_STORE_F32 ? 0 : qnn_words(store, C);
    rc = qnn_side_quantize(w, kernel, kh * kw * w->cout, bias, w->cout, s);
    if (rc == QNN_OK) rc = pack_pairs(w, s);
    if (rc == QNN_OK) rc = qnn_side_hip(hipGetLastError(), "hipGetLastError()");
    if (rc != QNN_OK) {
        qnn_depthwise_free(w);
        return rc;
    }
    *out = w;
    return QNN_OK;
}

extern "C" int qnn_depthwise_free(qnn_dw_weights_t* w) {
    if (!w) return QNN_OK;
    if (w->d_wpk) (void)hipFree(w->d_wpk);
    qnn_side_free(w);
    delete w;
    return QNN_OK;
}

extern "C" int qnn_depthwise_dequant(const qnn_dw_weights_t* w, float* kernel_khkwCM, void* stream) {
    QNN_REQUIRE(w && kernel_khkwCM, QNN_EINVAL, "qnn_depthwise_dequant: null pointer");
    QNN_HIP(hipMemcpyAsync(kernel_khkwCM, w->d_wq, (size_t)w->kh * w->kw * w->cout * sizeof(float),
                           hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return QNN_OK;
}

extern "C" int qnn_depthwise_out_hw(const qnn_dw_weights_t* w, int H, int W, int* Ho, int* Wo) {
    QNN_REQUIRE(w && Ho && Wo, QNN_EINVAL, "qnn_depthwise_out_hw: null pointer");
    QNN_REQUIRE(H > 0 && W > 0, QNN_EINVAL, "qnn_depthwise_out_hw: image %dx%d", H, W);
    DwGeom g;
    out_hw(w, H, W, &g);
    *Ho = g.Ho;
    *Wo = g.Wo;
    return QNN_OK;
}

extern "C" int qnn_depthwise_forward(const qnn_dw_weights_t* w, const void* x, int x_store, int x_bits, int N, int H,
                                     int W, const qnn_epilogue_t* epi, void* y, void* stream) {
    const char* who = "qnn_depthwise_forward";
    QNN_REQUIRE(w && epi, QNN_EINVAL, "%s: null handle or epilogue", who);
    QNN_REQUIRE(N >= 0 && H > 0 && W > 0, QNN_EINVAL, "%s: N=%d H=%d W=%d", who, N, H, W);
    int xshift;
    EpiArgs e;
    int rc = qnn_side_forward_check(who, w, w->cout, x_store, x_bits, epi, "a depthwise layer", &xshift, &e);
    if (rc != QNN_OK) return rc;
    const bool packed = x_store != QNN_STORE_F32;
    // ---- geometry ----
    DwGeom g;
    out_hw(w, H, W, &g);
    QNN_REQUIRE(g.Ho > 0 && g.Wo > 0, QNN_EINVAL, "%s: empty output (%dx%d image, effective window %dx%d)", who, H, W,
                w->dil_h * (w->kh - 1) + 1, w->dil_w * (w->kw - 1) + 1);
    g.H = H; g.W = W; g.C = w->C; g.M = w->M; g.cout = w->cout;
    g.kh = w->kh; g.kw = w->kw; g.stride = w->stride; g.dil_h = w->dil_h; g.dil_w = w->dil_w;
    g.xcw = packed ? w->xcw : w->C;
    g.ocw = e.ocw;
    bool run;
    rc = qnn_side_io_check(who, N, (size_t)N * g.Ho * g.Wo * (size_t)g.ocw, x, (size_t)N * H * W * g.xcw * 4, y, &run);
    if (!run) return rc;

    const bool fast = packed && e.out_store == x_store && pk16_ok(w, x_bits);
    const bool aligned = (uintptr_t)x % 16 == 0 && (uintptr_t)y % 16 == 0;
    // the 16-bit-lane form: one word per lane and kRows output rows per item; the plain form: V words of one pixel
    const bool v4 = !fast && aligned && g.ocw % 4 == 0;
    g.groups = fast ? g.ocw : v4 ? g.ocw / 4 : g.ocw;
    const int yblocks = fast ? (g.Ho + kRows - 1) / kRows : g.Ho;
    g.fd_g = qnn_fastdiv((uint32_t)g.groups);
    g.fd_wo = qnn_fastdiv((uint32_t)g.Wo);
    g.fd_ho = qnn_fastdiv((uint32_t)yblocks);
    g.fd_m = qnn_fastdiv((uint32_t)g.M);
    const uint32_t total = (uint32_t)((size_t)N * yblocks * g.Wo * (size_t)g.groups);
    hipStream_t s = (hipStream_t)stream;
    if (fast) {
        if (x_store == QNN_STORE_I4) launch_pk16<QNN_STORE_I4>(e.fn, x, w, y, g, e, total, s);
        else launch_pk16<QNN_STORE_I8>(e.fn, x, w, y, g, e, total, s);
    } else {
        qnn_side_for_store(x_store, [&](auto xs) { launch_plain<decltype(xs)::value>(v4, x, w, y, g, e, total, s); });
    }
    QNN_HIP(hipGetLastError());
    qnn_side_kernel_name("depthwise", x_store, fast ? "" : "_plain");
    return QNN_OK;
}
