// Keras Conv2DTranspose with float, binary, quantized or ternary weights (include/qnn_abi_tconv.h) on float32 tensors and
// on packed codes, in GATHER form: output row oy is reached by the taps ky == (oy + pad_before) mod s from input row
// iy = (oy + pad_before - ky) / s, so every output value is one sum -- no atomics, no scatter.  The integer arithmetic of
// the conv kernels and the shared float32 chain (qnn_epi_value / qnn_epi_code, qnn_common.h) behind it.
//
// k_tc_plain -- any window, stride, padding, store and channel count; 32-bit (float32 input: float64) sums.  qnn_pool.hip's
// lane map: one lane owns V consecutive 32-bit words (float32 output: V consecutive channels) of ONE output pixel,
// consecutive lanes own the next groups of that pixel and then of the next pixel.  V = 4 (16 bytes per lane) where the
// words per pixel divide by 4 and both pointers are 16-byte aligned, V = 1 otherwise.  It is the correctness form: per
// output channel and tap it walks the input pixel's words against the filter's words (prepacked in the input's store
// layout with zero spare bits, so whatever x holds in its spare bits meets a zero weight).
//
// k_tc_mfma -- stride 2, square windows 2 / 3 / 4, I4 / I8 codes in and out, Cin % 64 == 0, Cout % 16 == 0, on
// v_mfma_i32_16x16x64_i8.  Sub-pixel phases: the output pixels of one image with the same (row parity, column parity)
// read their input through one fixed list of 1 .. 4 taps (jy, jx): input pixel (by - jy, bx - jx), where (by, bx)
// advances by one input pixel per output pixel of the phase.  A wave takes kPG groups of 16 such pixels (flattened over
// the phase's rows of ONE image) x 32 filters: per tap and 64-channel K-step it loads the two filter tiles once (A,
// prepacked per phase and tap in operand order by k_tc_mfma_image) and per group the lanes' 16 channels of their pixel
// (B; int4 widened to code * 16 bytes as the strip kernels do, the 1/16 folded into the output scale), one MFMA per tile.
// A tap outside the image is read through the image's buffer descriptor at an out-of-range offset: a zero operand, no
// branch.  Filter row r of tile nt is filter fbase + 8 * (r >> 2) + 4 * nt + (r & 3), so a lane ends with the 8
// CONSECUTIVE filters fbase + 8 * (lane >> 4) .. + 7 of its pixel: one int4 word or two int8 words, stored without a
// transpose.  No LDS.
//
// Index arithmetic in 32 bits by multiply-high (the entry refuses 2^31 output words), tensor offsets in 64 bits.
#include <new>

#include "qnn_sideconv.h"
#include "qnn_strip_device.h"
#include "qnn_abi_tconv.h"

struct qnn_tconv_weights : SideWeights {   // d_wq, d_wcode: [kh*kw][cout][cin], Keras' (kh, kw, Cout, Cin) order
    int kh, kw, cout, cin;
    int stride, same_pad;
    uint32_t* d_wpk;         // [kh*kw][cout][xcw] codes packed like an input pixel, spare bits zero, or nullptr
    uint8_t* d_wm;           // matrix-pipe image [phase 4][tap 4][K-step][32-filter block][tile 2][lane 64][16 bytes], or nullptr
};

namespace {

constexpr int kBlock = 256;
constexpr int kPG = 4;       // 16-pixel groups a wave of k_tc_mfma takes per filter load

// ---- weights ----------------------------------------------------------------------------------------------------------
// word wi of filter row (tap, f) in the layout of an input pixel on `store`; channels beyond cin - 1 stay zero
__global__ __launch_bounds__(kBlock) void k_tc_pack_words(const int32_t* __restrict__ wcode, uint32_t* __restrict__ wpk,
                                                          int rows, int cin, int xcw, int store) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= rows * xcw) return;
    const int row = i / xcw, wi = i - row * xcw;
    const int32_t* src = wcode + (size_t)row * cin;
    uint32_t word = 0;
    if (store == QNN_STORE_T2) {             // (mask, sign) word pairs
        const int c0 = (wi >> 1) * 32;
        for (int j = 0; j < 32 && c0 + j < cin; ++j) {
            const int code = src[c0 + j];
            word |= (uint32_t)((wi & 1) ? code > 0 : code != 0) << j;
        }
    } else {
        const int pw = qnn_per_word(store), bits = 32 / pw;
        const uint32_t mask = (1u << bits) - 1u;
        for (int j = 0; j < pw && wi * pw + j < cin; ++j) {
            const int code = src[wi * pw + j];
            word |= (store == QNN_STORE_BIN ? (uint32_t)(code > 0) : ((uint32_t)code & mask)) << (j * bits);
        }
    }
    wpk[i] = word;
}

// ---- the sub-pixel phases of stride 2 -----------------------------------------------------------------------------------
// Output parity class rp (oy = 2 * yr + rp): kernel-row phase py = (rp + pb) & 1, the taps are ky = py + 2 * jy < k and read
// input row yr + ((rp + pb) >> 1) - jy.  The same rule for columns.
__host__ __device__ inline int tc_phase(int par, int pb) { return (par + pb) & 1; }
__host__ __device__ inline int tc_base(int par, int pb) { return (par + pb) >> 1; }
__host__ __device__ inline int tc_ntaps(int k, int phase) { return (k - phase + 1) >> 1; }

// One byte per thread of the image [phase rp * 2 + cp][tap jy * 2 + jx][kc][fb][nt][lane][16]: the weight code (int8) of
// filter fb * 32 + 8 * (r >> 2) + 4 * nt + (r & 3) and channel kc * 64 + 16 * kq + qnn_operand_channel(j); zero for a tap
// the phase does not have and for a filter beyond cout - 1.
__global__ __launch_bounds__(kBlock) void k_tc_mfma_image(const int32_t* __restrict__ wcode, uint8_t* __restrict__ wm, int k,
                                                          int pb, int cout, int cin, int store, uint32_t total) {
    const uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (i >= total) return;
    const int KC = cin / 64, FB = (cout + 31) / 32;
    uint32_t t = i;
    const int j = t & 15; t >>= 4;
    const int lane = t & 63; t >>= 6;
    const int nt = t & 1; t >>= 1;
    const int fb = t % FB; t /= FB;
    const int kc = t % KC; t /= KC;
    const int tap = t & 3, ph = t >> 2;
    const int r = lane & 15, kq = lane >> 4;
    const int ky = tc_phase(ph >> 1, pb) + 2 * (tap >> 1), kx = tc_phase(ph & 1, pb) + 2 * (tap & 1);
    const int f = fb * 32 + 8 * (r >> 2) + 4 * nt + (r & 3);
    const int c = kc * 64 + 16 * kq + qnn_operand_channel(store, j);
    int code = 0;
    if (ky < k && kx < k && f < cout) code = wcode[((size_t)(ky * k + kx) * cout + f) * cin + c];
    wm[i] = (uint8_t)(int8_t)code;
}

// ---- geometry ---------------------------------------------------------------------------------------------------------
struct TcGeom {
    int H, W, Ho, Wo, cin, cout;
    int kh, kw, stride, pt, pl;
    int xcw;                   // words (float32: channels) per input pixel
    int ocw;                   // words (float32: channels) per output pixel
    int groups;                // items per output pixel = ocw / V
    FastDiv fd_g, fd_wo, fd_ho, fd_s;
};

struct Item {
    uint32_t q;                // output pixel (n, oy, ox) flattened
    int g, n, fy, fx;          // word group; image; the pixel's row and column in `full`
};

__device__ __forceinline__ Item decode(uint32_t i, const TcGeom& p) {
    Item it;
    it.q = qnn_div(i, p.fd_g);
    it.g = (int)(i - it.q * (uint32_t)p.groups);
    const uint32_t t = qnn_div(it.q, p.fd_wo);
    const int ox = (int)(it.q - t * (uint32_t)p.Wo);
    it.n = (int)qnn_div(t, p.fd_ho);
    const int oy = (int)(t - (uint32_t)it.n * (uint32_t)p.Ho);
    it.fy = oy + p.pt;
    it.fx = ox + p.pl;
    return it;
}

// sum over the cin channels of one packed pixel `px` x one packed filter row `wr` (spare bits of wr are zero)
template <int XS>
__device__ __forceinline__ int dot_pixel(const uint32_t* __restrict__ px, const uint32_t* __restrict__ wr, int xcw, int cin,
                                         int acc) {
    if constexpr (XS == QNN_STORE_BIN) {
        // +-1 x +-1 over the valid bits: n - 2 popcount((a ^ w) & valid)
        for (int wi = 0; wi < xcw; ++wi) {
            const int nb = min(32, cin - 32 * wi);
            const uint32_t valid = nb == 32 ? 0xFFFFFFFFu : (1u << nb) - 1u;
            acc += nb - 2 * __popc((px[wi] ^ wr[wi]) & valid);
        }
    } else if constexpr (XS == QNN_STORE_T2) {
        for (int wi = 0; wi < xcw; wi += 2) acc = qnn_dot_t2(px[wi], px[wi + 1], wr[wi], wr[wi + 1], acc);
    } else {
        for (int wi = 0; wi < xcw; ++wi) acc = qnn_dot<XS>(px[wi], wr[wi], acc);
    }
    return acc;
}

// ---- the plain form ---------------------------------------------------------------------------------------------------
// XS: the input's store.  The output's store is e.out_store (wave-uniform).  A lane walks its V output words, the
// channels of a word and the contributing taps of the pixel; a channel beyond cout - 1 is left out, so its bits stay zero.
template <int XS, int V>
__global__ __launch_bounds__(kBlock) void k_tc_plain(const void* __restrict__ x, const float* __restrict__ wq,
                                                     const uint32_t* __restrict__ wpk, void* __restrict__ y,
                                                     const TcGeom p, const EpiArgs e, const uint32_t total) {
    const uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (i >= total) return;
    const Item it = decode(i, p);
    const int w0 = it.g * V;
    const int opw = qnn_per_word(e.out_store), obits = 32 / opw;
    const uint32_t omask = obits == 32 ? 0xFFFFFFFFu : (1u << obits) - 1u;
    // first contributing tap of each axis and its input cell; the next taps are s further and one cell back
    const int qy = (int)qnn_div((uint32_t)it.fy, p.fd_s), ky0 = it.fy - qy * p.stride;
    const int qx = (int)qnn_div((uint32_t)it.fx, p.fd_s), kx0 = it.fx - qx * p.stride;
    uint32_t out[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        uint32_t word = 0;
        for (int j = 0; j < opw; ++j) {
            const int oc = (w0 + v) * opw + j;
            if (oc >= p.cout) break;
            double facc = 0.0;
            int acc = 0;
            for (int ky = ky0, iy = qy; ky < p.kh && iy >= 0; ky += p.stride, --iy) {
                if (iy >= p.H) continue;
                for (int kx = kx0, ix = qx; kx < p.kw && ix >= 0; kx += p.stride, --ix) {
                    if (ix >= p.W) continue;
                    const size_t pix = ((size_t)it.n * p.H + iy) * p.W + ix;
                    const size_t row = (size_t)(ky * p.kw + kx) * p.cout + oc;
                    if constexpr (XS == QNN_STORE_F32) {
                        const float* a = (const float*)x + pix * p.cin;
                        const float* wr = wq + row * p.cin;
                        for (int c = 0; c < p.cin; ++c) facc += (double)a[c] * (double)wr[c];
                    } else {
                        acc = dot_pixel<XS>((const uint32_t*)x + pix * p.xcw, wpk + row * p.xcw, p.xcw, p.cin, acc);
                    }
                }
            }
            float val = XS == QNN_STORE_F32 ? (float)facc : __fmul_rn((float)acc, e.scale);
            val = qnn_epi_value(val, oc, e);
            if (e.out_store == QNN_STORE_F32) word = __float_as_uint(act_value(val, e));
            else word |= ((uint32_t)qnn_epi_code(val, e) & omask) << (j * obits);
        }
        out[v] = word;
    }
    store_words<V>((uint32_t*)y + (size_t)it.q * p.ocw + w0, out);
}

// ---- the matrix-pipe form -----------------------------------------------------------------------------------------------
struct TcMfma {
    int H, W, Ho, Wo, cout;
    int k, pb;                 // window, pad_before (both axes)
    int KC, FB;                // 64-channel K-steps, 32-filter blocks
    int GT;                    // wave tasks per (image, phase, filter block): ceil(groups of the largest phase / kPG)
    uint32_t img_bytes;        // one input image as stored
    uint32_t waves;            // N * 4 * GT * FB
    FastDiv fd_fb, fd_gt, fd_wp[2];
};

// XS = I4 / I8 (input and output store).  wave task = (image n, phase rp * 2 + cp, kPG groups from g0, filter block fb),
// fb fastest: the waves that read the same pixels run next to each other.
template <int XS>
__global__ __launch_bounds__(kBlock) void k_tc_mfma(const uint8_t* __restrict__ x, const uint8_t* __restrict__ wm,
                                                    uint32_t* __restrict__ y, const TcMfma p, const EpiArgs e) {
    constexpr int LB = XS == QNN_STORE_I4 ? 8 : 16;       // bytes a lane loads per K-step: its 16 channels
    constexpr int OW = XS == QNN_STORE_I4 ? 1 : 2;        // output words per lane: 8 consecutive filters
    constexpr int OB = XS == QNN_STORE_I4 ? 4 : 8;
    const int lane = threadIdx.x & 63;
    const int r = lane & 15, kq = lane >> 4;
    const uint32_t wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)));
    if (wave >= p.waves) return;
    uint32_t t = qnn_div(wave, p.fd_fb);
    const int fb = (int)(wave - t * (uint32_t)p.FB);
    const uint32_t t2 = qnn_div(t, p.fd_gt);
    const int g0 = (int)(t - t2 * (uint32_t)p.GT) * kPG;
    const int ph = (int)(t2 & 3u), n = (int)(t2 >> 2);
    const int rp = ph >> 1, cp = ph & 1;
    const int Hp = (p.Ho - rp + 1) >> 1, Wp = (p.Wo - cp + 1) >> 1;      // the phase's output rows and columns
    const int npix = Hp * Wp;
    if (g0 * 16 >= npix) return;                                        // wave-uniform: a smaller phase has fewer groups
    const int nty = tc_ntaps(p.k, tc_phase(rp, p.pb)), ntx = tc_ntaps(p.k, tc_phase(cp, p.pb));
    const int by0 = tc_base(rp, p.pb), bx0 = tc_base(cp, p.pb);
    const int pixb = p.KC * 4 * LB;                                     // bytes per stored input pixel

    // the lane's pixel of every group: (yr, m) in the phase, its input cell at tap (0, 0), its output pixel
    int by[kPG], bx[kPG];
    bool valid[kPG];
    size_t opix[kPG];
#pragma unroll
    for (int pg = 0; pg < kPG; ++pg) {
        const int pi = (g0 + pg) * 16 + r;
        valid[pg] = pi < npix;
        const int yr = (int)qnn_div((uint32_t)pi, p.fd_wp[cp]);
        const int m = pi - yr * Wp;
        by[pg] = yr + by0;
        bx[pg] = m + bx0;
        opix[pg] = ((size_t)n * p.Ho + (2 * yr + rp)) * p.Wo + (2 * m + cp);
    }
    const __amdgpu_buffer_rsrc_t xr = strip_image_rsrc(x, n, p.img_bytes);
    const v4i* wv = reinterpret_cast<const v4i*>(wm);

    v4i acc[kPG][2];
#pragma unroll
    for (int pg = 0; pg < kPG; ++pg) acc[pg][0] = acc[pg][1] = v4i{0, 0, 0, 0};

    for (int jy = 0; jy < nty; ++jy)
        for (int jx = 0; jx < ntx; ++jx) {
            // byte offset of the lane's 16 channels of K-step 0; a cell outside the image (or a pixel beyond the phase)
            // sits at an out-of-range offset and stays there: the descriptor returns zeros
            int voff[kPG];
#pragma unroll
            for (int pg = 0; pg < kPG; ++pg) {
                const int iy = by[pg] - jy, ix = bx[pg] - jx;
                const bool ok = valid[pg] && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
                voff[pg] = ok ? (iy * p.W + ix) * pixb + kq * LB : (int)0x80000000;
            }
            const v4i* wt = wv + ((size_t)((ph * 4 + jy * 2 + jx) * p.KC) * p.FB + fb) * 128 + lane;
            for (int kc = 0; kc < p.KC; ++kc) {
                const v4i a0 = wt[0], a1 = wt[64];
                wt += (size_t)p.FB * 128;
                v4i b[kPG];
#pragma unroll
                for (int pg = 0; pg < kPG; ++pg) {
                    if constexpr (XS == QNN_STORE_I4) {
                        b[pg] = strip_widen(__builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(xr, voff[pg], 0, 0)));
                    } else {
                        b[pg] = __builtin_bit_cast(v4i, __builtin_amdgcn_raw_buffer_load_b128(xr, voff[pg], 0, 0));
                    }
                    voff[pg] += 4 * LB;                                  // out of range stays out of range: < 2^31 steps
                }
#pragma unroll
                for (int pg = 0; pg < kPG; ++pg) {
                    acc[pg][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, b[pg], acc[pg][0], 0, 0, 0);
                    acc[pg][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, b[pg], acc[pg][1], 0, 0, 0);
                }
            }
        }

    // the lane's 8 consecutive filters: constants once, then the shared chain per value
    const int f0 = fb * 32 + 8 * kq;
    if (f0 >= p.cout) return;                                           // cout % 16 == 0: all 8 in or all 8 out
    float cb[8], ci[8], cs[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        cb[j] = e.bias ? e.bias[f0 + j] : 0.0f;
        ci[j] = e.bn_inv ? e.bn_inv[f0 + j] : 1.0f;
        cs[j] = e.bn_inv ? e.bn_shift[f0 + j] : 0.0f;
    }
    EpiArgs le = e;
    le.trick_s = 0.0f;
    le.bias = e.bias ? cb : nullptr;
    le.bn_inv = e.bn_inv ? ci : nullptr;
    le.bn_shift = cs;
    constexpr uint32_t MASK = (1u << OB) - 1u;
#pragma unroll
    for (int pg = 0; pg < kPG; ++pg) {
        uint32_t wd[OW];
#pragma unroll
        for (int o = 0; o < OW; ++o) wd[o] = 0;
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int j = 4 * nt + i;
                const float val = qnn_epi_value(__fmul_rn((float)acc[pg][nt][i], e.scale), j, le);
                const uint32_t code = (uint32_t)qnn_epi_code(val, le) & MASK;
                if constexpr (XS == QNN_STORE_I4) wd[0] |= code << (4 * j);
                else wd[nt] |= code << (8 * i);
            }
        if (valid[pg]) {
            uint32_t* dst = y + opix[pg] * (size_t)e.ocw + (size_t)f0 * OB / 32;
            if constexpr (OW == 1) dst[0] = wd[0];
            else *reinterpret_cast<uint2*>(dst) = make_uint2(wd[0], wd[1]);
        }
    }
}

// THE route rule of the matrix-pipe form (include/qnn_abi_tconv.h states it; tests/tconv_cases.py restates it).  The
// handle's half is asked with x == y == nullptr at prepack: it decides whether the operand image is built.
bool mfma_ok(int kh, int kw, int stride, int store, int cout, int cin, int x_store, int out_store, int H, int W,
             const void* x, const void* y) {
    if (stride != 2 || kh != kw || kh < 2 || kh > 4) return false;
    if ((store != QNN_STORE_I4 && store != QNN_STORE_I8) || x_store != store || out_store != x_store) return false;
    if (cin % 64 != 0 || cin > 16384 || cout % 16 != 0) return false;
    if ((uintptr_t)x % 16 != 0 || (uintptr_t)y % 16 != 0) return false;
    return (size_t)H * W * (size_t)qnn_words(store, cin) * 4 < ((size_t)1 << 31);
}

template <int XS>
void launch_plain(bool v4, const void* x, const qnn_tconv_weights* w, void* y, const TcGeom& g, const EpiArgs& e,
                  uint32_t total, hipStream_t s) {
    const dim3 grid((total + kBlock - 1) / kBlock), block(kBlock);
    if (v4) hipLaunchKernelGGL((k_tc_plain<XS, 4>), grid, block, 0, s, x, w->d_wq, w->d_wpk, y, g, e, total);
    else hipLaunchKernelGGL((k_tc_plain<XS, 1>), grid, block, 0, s, x, w->d_wq, w->d_wpk, y, g, e, total);
}

void out_hw(const qnn_tconv_weights* w, int H, int W, TcGeom* g) {
    qnn_tconv_out_pad(H, w->kh, w->stride, w->same_pad, &g->Ho, &g->pt);
    qnn_tconv_out_pad(W, w->kw, w->stride, w->same_pad, &g->Wo, &g->pl);
}

// prepack: the filter rows of the plain form on a packed store, and the operand image where the shape takes the matrix pipe
int pack_images(qnn_tconv_weights* w, hipStream_t s) {
    if (w->store != QNN_STORE_F32) {
        const int rows = w->kh * w->kw * w->cout, nw = rows * w->xcw;
        QNN_SIDE_HIP(hipMalloc(&w->d_wpk, (size_t)nw * sizeof(uint32_t)));
        hipLaunchKernelGGL(k_tc_pack_words, dim3((nw + kBlock - 1) / kBlock), dim3(kBlock), 0, s, w->d_wcode, w->d_wpk, rows,
                           w->cin, w->xcw, w->store);
    }
    if (mfma_ok(w->kh, w->kw, w->stride, w->store, w->cout, w->cin, w->store, w->store, 1, 1, nullptr, nullptr)) {
        int ho, pb;
        qnn_tconv_out_pad(1, w->kh, w->stride, w->same_pad, &ho, &pb);
        const uint32_t total = 16u * (uint32_t)(w->cin / 64) * (uint32_t)((w->cout + 31) / 32) * 2u * 64u * 16u;
        QNN_SIDE_HIP(hipMalloc(&w->d_wm, (size_t)total));
        hipLaunchKernelGGL(k_tc_mfma_image, dim3((total + kBlock - 1) / kBlock), dim3(kBlock), 0, s, w->d_wcode, w->d_wm, w->kh,
                           pb, w->cout, w->cin, w->store, total);
    }
    return QNN_OK;
}

}  // namespace

extern "C" int qnn_tconv_prepack(int wkind, int wbits, float H, const float* kernel, int kh, int kw, int Cout, int Cin,
                                 const float* bias, int stride, int same_pad, int store, void* stream,
                                 qnn_tconv_weights_t** out) {
    const char* who = "qnn_tconv_prepack";
    QNN_REQUIRE(kernel && out, QNN_EINVAL, "%s: null pointer", who);
    QNN_REQUIRE(stride >= 1, QNN_EINVAL, "%s: stride=%d", who, stride);
    QNN_REQUIRE(stride <= QNN_TC_MAX_STRIDE, QNN_EUNSUPPORTED, "%s: stride=%d (1 .. %d)", who, stride, QNN_TC_MAX_STRIDE);
    QNN_REQUIRE(kh > 0 && kw > 0 && Cout > 0 && Cin > 0, QNN_EINVAL, "%s: kernel shape (%d,%d,%d,%d)", who, kh, kw, Cout, Cin);
    QNN_REQUIRE(kh <= QNN_TC_MAX_WINDOW, QNN_EUNSUPPORTED, "%s: kh=%d above QNN_TC_MAX_WINDOW = %d", who, kh, QNN_TC_MAX_WINDOW);
    QNN_REQUIRE(kw <= QNN_TC_MAX_WINDOW, QNN_EUNSUPPORTED, "%s: kw=%d above QNN_TC_MAX_WINDOW = %d", who, kw, QNN_TC_MAX_WINDOW);
    QNN_REQUIRE((double)Cout * Cin * kh * kw < 1.0e9, QNN_EUNSUPPORTED, "%s: %d x %d channels", who, Cout, Cin);
    SideWeights common{};
    int rc = qnn_side_weights_check(who, wkind, wbits, H, store, &common);
    if (rc != QNN_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    qnn_tconv_weights* w = new (std::nothrow) qnn_tconv_weights();
    QNN_REQUIRE(w, QNN_ENOMEM, "%s: host allocation failed", who);
    *static_cast<SideWeights*>(w) = common;
    w->kh = kh; w->kw = kw; w->cout = Cout; w->cin = Cin;
    w->stride = stride; w->same_pad = same_pad ? 1 : 0;
    w->xcw = store == QNN_STORE_F32 ? 0 : qnn_words(store, Cin);
    rc = qnn_side_quantize(w, kernel, kh * kw * Cout * Cin, bias, Cout, s);
    if (rc == QNN_OK) rc = pack_images(w, s);
    if (rc == QNN_OK) rc = qnn_side_hip(hipGetLastError(), "hipGetLastError()");
    if (rc != QNN_OK) {
        qnn_tconv_free(w);
        return rc;
    }
    *out = w;
    return QNN_OK;
}

extern "C" int qnn_tconv_free(qnn_tconv_weights_t* w) {
    if (!w) return QNN_OK;
    if (w->d_wpk) (void)hipFree(w->d_wpk);
    if (w->d_wm) (void)hipFree(w->d_wm);
    qnn_side_free(w);
    delete w;
    return QNN_OK;
}

extern "C" int qnn_tconv_dequant(const qnn_tconv_weights_t* w, float* kernel_khkwFC, void* stream) {
    QNN_REQUIRE(w && kernel_khkwFC, QNN_EINVAL, "qnn_tconv_dequant: null pointer");
    QNN_HIP(hipMemcpyAsync(kernel_khkwFC, w->d_wq, (size_t)w->kh * w->kw * w->cout * w->cin * sizeof(float),
                           hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return QNN_OK;
}

extern "C" int qnn_tconv_out_hw(const qnn_tconv_weights_t* w, int H, int W, int* Ho, int* Wo) {
    QNN_REQUIRE(w && Ho && Wo, QNN_EINVAL, "qnn_tconv_out_hw: null pointer");
    QNN_REQUIRE(H > 0 && W > 0, QNN_EINVAL, "qnn_tconv_out_hw: image %dx%d", H, W);
    QNN_REQUIRE(H < (1 << 26) && W < (1 << 26), QNN_EINVAL, "qnn_tconv_out_hw: image %dx%d", H, W);
    TcGeom g;
    out_hw(w, H, W, &g);
    *Ho = g.Ho;
    *Wo = g.Wo;
    return QNN_OK;
}

extern "C" int qnn_tconv_forward(const qnn_tconv_weights_t* w, const void* x, int x_store, int x_bits, int N, int H, int W,
                                 const qnn_epilogue_t* epi, void* y, void* stream) {
    const char* who = "qnn_tconv_forward";
    QNN_REQUIRE(w && epi, QNN_EINVAL, "%s: null handle or epilogue", who);
    QNN_REQUIRE(N >= 0 && H > 0 && W > 0 && H < (1 << 26) && W < (1 << 26), QNN_EINVAL, "%s: N=%d H=%d W=%d", who, N, H, W);
    int xshift;
    EpiArgs e;
    int rc = qnn_side_forward_check(who, w, w->cout, x_store, x_bits, epi, "a transposed convolution", &xshift, &e);
    if (rc != QNN_OK) return rc;
    const bool packed = x_store != QNN_STORE_F32;
    // ---- the int32 bound: the most (tap, channel) pairs one output value sums, each at most 2^(x_bits-1) * 2^wshift ----
    if (packed) {
        const int s = w->stride;
        const double worst = (double)((w->kh + s - 1) / s) * ((w->kw + s - 1) / s) * w->cin * (double)(1u << xshift) *
                             (double)(1u << w->wshift);
        QNN_REQUIRE(worst < 2147483648.0, QNN_EUNSUPPORTED,
                    "%s: the int32 sum could overflow: ceil(kh/s) * ceil(kw/s) * Cin * 2^(x_bits-1) * 2^wshift = %.0f (2^31 or more)",
                    who, worst);
    }
    // ---- geometry ----
    TcGeom g;
    out_hw(w, H, W, &g);
    g.H = H; g.W = W; g.cin = w->cin; g.cout = w->cout;
    g.kh = w->kh; g.kw = w->kw; g.stride = w->stride;
    g.xcw = packed ? w->xcw : w->cin;
    g.ocw = e.ocw;
    bool run;
    rc = qnn_side_io_check(who, N, (size_t)N * g.Ho * g.Wo * (size_t)g.ocw, x, (size_t)N * H * W * g.xcw * 4, y, &run);
    if (!run) return rc;

    hipStream_t s = (hipStream_t)stream;
    const bool fast = packed && w->d_wm &&
                      mfma_ok(w->kh, w->kw, w->stride, w->store, w->cout, w->cin, x_store, e.out_store, H, W, x, y);
    if (fast) {
        TcMfma p{};
        p.H = H; p.W = W; p.Ho = g.Ho; p.Wo = g.Wo; p.cout = w->cout;
        p.k = w->kh; p.pb = g.pt;
        p.KC = w->cin / 64; p.FB = (w->cout + 31) / 32;
        const int groups = (((g.Ho + 1) / 2) * ((g.Wo + 1) / 2) + 15) / 16;      // of phase (0, 0), the largest
        p.GT = (groups + kPG - 1) / kPG;
        p.img_bytes = (uint32_t)((size_t)H * W * w->xcw * 4);
        const size_t waves = (size_t)N * 4 * p.GT * p.FB;                       // <= output words: below 2^31
        p.waves = (uint32_t)waves;
        p.fd_fb = qnn_fastdiv((uint32_t)p.FB);
        p.fd_gt = qnn_fastdiv((uint32_t)p.GT);
        p.fd_wp[0] = qnn_fastdiv((uint32_t)((g.Wo + 1) / 2));
        p.fd_wp[1] = qnn_fastdiv((uint32_t)(g.Wo / 2 > 0 ? g.Wo / 2 : 1));
        if (x_store == QNN_STORE_I4) e.scale = ldexpf(e.scale, -4);              // operands are code * 16
        const dim3 grid((uint32_t)((waves + kBlock / 64 - 1) / (kBlock / 64))), block(kBlock);
        if (x_store == QNN_STORE_I4)
            hipLaunchKernelGGL((k_tc_mfma<QNN_STORE_I4>), grid, block, 0, s, (const uint8_t*)x, w->d_wm, (uint32_t*)y, p, e);
        else
            hipLaunchKernelGGL((k_tc_mfma<QNN_STORE_I8>), grid, block, 0, s, (const uint8_t*)x, w->d_wm, (uint32_t*)y, p, e);
    } else {
        const bool v4 = (uintptr_t)x % 16 == 0 && (uintptr_t)y % 16 == 0 && g.ocw % 4 == 0;
        g.groups = v4 ? g.ocw / 4 : g.ocw;
        g.fd_g = qnn_fastdiv((uint32_t)g.groups);
        g.fd_wo = qnn_fastdiv((uint32_t)g.Wo);
        g.fd_ho = qnn_fastdiv((uint32_t)g.Ho);
        g.fd_s = qnn_fastdiv((uint32_t)g.stride);
        const uint32_t total = (uint32_t)((size_t)N * g.Ho * g.Wo * (size_t)g.groups);
        qnn_side_for_store(x_store, [&](auto xs) { launch_plain<decltype(xs)::value>(v4, x, w, y, g, e, total, s); });
    }
    QNN_HIP(hipGetLastError());
    qnn_side_kernel_name("tconv", x_store, fast ? "_mfma" : "_plain");
    return QNN_OK;
}
