// Keras MaxPooling2D / AveragePooling2D with pool_size, strides and padding (include/qnn_abi_pool.h) on float32 tensors
// and on packed codes.  The maximum of grid codes is a grid code, so a max-pool between two low-bit layers maps packed
// words to packed words and the activation never exists in float32.
//
// Memory-bound, no reuse worth an LDS stage: every input word is read by at most ceil(ph / sh) * ceil(pw / sw) windows
// and those re-reads hit L2.  One lane owns V consecutive 32-bit words (float32: V consecutive channels) of ONE output
// pixel, consecutive lanes own consecutive groups of that pixel and then of the next pixel: a wave reads, per tap, runs
// of whole pixels, V = 4 (16 bytes per lane, global_load_dwordx4) where the words per pixel divide by 4 and both
// pointers are 16-byte aligned, V = 1 otherwise.  Taps outside the image are cut off by the loop bounds: they are
// neither loaded nor replaced by a value.  One item per thread, index arithmetic in 32 bits by multiply-high (FastDiv):
// the entry refuses N * Ho * Wo * groups >= 2^31; tensor offsets are 64-bit.
#include <stdio.h>

#include "qnn_sideconv.h"
#include "qnn_abi_pool.h"

namespace {

constexpr int kBlock = 256;

struct PoolGeom {
    int H, W, Ho, Wo, C;
    int cw;                    // words (float32: channels) per pixel, of x and of a max-pool's y
    int groups;                // items per output pixel = cw / V
    int ph, pw, sh, sw, pt, pl;
    FastDiv fd_g, fd_wo, fd_ho;
};

struct Item {
    uint32_t q;                // output pixel (n, oy, ox) flattened
    int g;                     // word group inside the pixel
    int n;
    int ya, yb, xa, xb;        // the in-bounds part of the window: rows ya .. yb - 1, columns xa .. xb - 1
};

__device__ __forceinline__ Item decode(uint32_t i, const PoolGeom& p) {
    Item it;
    it.q = qnn_div(i, p.fd_g);
    it.g = (int)(i - it.q * (uint32_t)p.groups);
    const uint32_t t = qnn_div(it.q, p.fd_wo);
    const int ox = (int)(it.q - t * (uint32_t)p.Wo);
    it.n = (int)qnn_div(t, p.fd_ho);
    const int oy = (int)(t - (uint32_t)it.n * (uint32_t)p.Ho);
    const int y0 = oy * p.sh - p.pt, x0 = ox * p.sw - p.pl;
    it.ya = max(y0, 0);
    it.yb = min(y0 + p.ph, p.H);
    it.xa = max(x0, 0);
    it.xb = min(x0 + p.pw, p.W);
    return it;
}

template <int STORE> struct Lay {
    static constexpr int PW = (STORE == QNN_STORE_BIN) ? 32 : (STORE == QNN_STORE_I4) ? 8 : 4;
    static constexpr int BITS = 32 / PW;
};

// signed field j of a word (I4 / I8): one v_bfe_i32
template <int BITS>
__device__ __forceinline__ int field(uint32_t w, int j) {
    return (int)(w << (32 - BITS - j * BITS)) >> (32 - BITS);
}

// ---- max on packed words ------------------------------------------------------------------------------------------
// BIN: bit 1 = +1, so the maximum is the OR of the words.  I4 / I8: the maximum of the sign-extended fields, put back
// together at the end.  The fields of a pixel's last word beyond channel C - 1 are written as zero (qnn_pack_f32's form).
template <int STORE, int V>
__global__ __launch_bounds__(kBlock) void k_pool_max(const uint32_t* __restrict__ x, uint32_t* __restrict__ y,
                                                     const PoolGeom p, const uint32_t total) {
    constexpr int PW = Lay<STORE>::PW, BITS = Lay<STORE>::BITS;
    const uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (i >= total) return;
    const Item it = decode(i, p);
    const int w0 = it.g * V;
    uint32_t out[V];
    if constexpr (STORE == QNN_STORE_BIN) {
#pragma unroll
        for (int v = 0; v < V; ++v) out[v] = 0u;
        for (int yy = it.ya; yy < it.yb; ++yy) {
            const uint32_t* row = x + ((size_t)it.n * p.H + yy) * p.W * p.cw + w0;
            for (int xx = it.xa; xx < it.xb; ++xx) {
                uint32_t w[V];
                load_words<V>(row + (size_t)xx * p.cw, w);
#pragma unroll
                for (int v = 0; v < V; ++v) out[v] |= w[v];
            }
        }
    } else {
        int m[V * PW];
#pragma unroll
        for (int k = 0; k < V * PW; ++k) m[k] = -(1 << (BITS - 1));      // the smallest code: every window has a tap
        for (int yy = it.ya; yy < it.yb; ++yy) {
            const uint32_t* row = x + ((size_t)it.n * p.H + yy) * p.W * p.cw + w0;
            for (int xx = it.xa; xx < it.xb; ++xx) {
                uint32_t w[V];
                load_words<V>(row + (size_t)xx * p.cw, w);
#pragma unroll
                for (int v = 0; v < V; ++v)
#pragma unroll
                    for (int j = 0; j < PW; ++j) m[v * PW + j] = max(m[v * PW + j], field<BITS>(w[v], j));
            }
        }
        constexpr uint32_t MASK = (1u << BITS) - 1u;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            uint32_t o = 0;
#pragma unroll
            for (int j = 0; j < PW; ++j) o |= ((uint32_t)m[v * PW + j] & MASK) << (j * BITS);
            out[v] = o;
        }
    }
    const int left = p.C - (p.cw - 1) * PW;          // channels in the pixel's last word, 1 .. PW
    if (left < PW && w0 + V == p.cw) out[V - 1] &= (1u << (left * BITS)) - 1u;
    store_words<V>(y + (size_t)it.q * p.cw + w0, out);
}

// ---- average of packed codes -> float32 -----------------------------------------------------------------------------
// Exact integer window sums, one rounding in the scaling (exact: a power of two) and one in the division by the number of
// in-bounds taps, as k_avgpool_packed.  A lane writes the PW * V consecutive channels of its words.
template <int STORE, int V>
__global__ __launch_bounds__(kBlock) void k_pool_avg(const uint32_t* __restrict__ x, float* __restrict__ y,
                                                     const PoolGeom p, const uint32_t total, const float inv_m) {
    constexpr int PW = Lay<STORE>::PW, BITS = Lay<STORE>::BITS;
    const uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (i >= total) return;
    const Item it = decode(i, p);
    const int w0 = it.g * V;
    int acc[V * PW];
#pragma unroll
    for (int k = 0; k < V * PW; ++k) acc[k] = 0;
    for (int yy = it.ya; yy < it.yb; ++yy) {
        const uint32_t* row = x + ((size_t)it.n * p.H + yy) * p.W * p.cw + w0;
        for (int xx = it.xa; xx < it.xb; ++xx) {
            uint32_t w[V];
            load_words<V>(row + (size_t)xx * p.cw, w);
#pragma unroll
            for (int v = 0; v < V; ++v)
#pragma unroll
                for (int j = 0; j < PW; ++j) {
                    if constexpr (STORE == QNN_STORE_BIN) acc[v * PW + j] += (int)((w[v] >> j) & 1u);
                    else acc[v * PW + j] += field<BITS>(w[v], j);
                }
        }
    }
    const int count = (it.yb - it.ya) * (it.xb - it.xa);
    const float fc = (float)count;
    float* yo = y + (size_t)it.q * p.C;
    const int c0 = w0 * PW;
#pragma unroll
    for (int k = 0; k < V * PW; ++k) {
        const int sum = STORE == QNN_STORE_BIN ? 2 * acc[k] - count : acc[k];      // ones minus zeros: codes +-1
        if (c0 + k < p.C) yo[c0 + k] = __fdiv_rn(__fmul_rn((float)sum, inv_m), fc);
    }
}

// ---- float32 ----------------------------------------------------------------------------------------------------------
// max: fmaxf over the in-bounds taps.  avg: the window summed in float64 in row order, rounded once to float32, divided in
// float32 by the number of in-bounds taps.
template <int MODE, int V>
__global__ __launch_bounds__(kBlock) void k_pool_f32(const float* __restrict__ x, float* __restrict__ y, const PoolGeom p,
                                                     const uint32_t total) {
    const uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (i >= total) return;
    const Item it = decode(i, p);
    const int c0 = it.g * V;
    float mx[V];
    double sum[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        mx[v] = -__builtin_huge_valf();
        sum[v] = 0.0;
    }
    for (int yy = it.ya; yy < it.yb; ++yy) {
        const float* row = x + ((size_t)it.n * p.H + yy) * p.W * p.cw + c0;
        for (int xx = it.xa; xx < it.xb; ++xx) {
            uint32_t w[V];
            load_words<V>(reinterpret_cast<const uint32_t*>(row + (size_t)xx * p.cw), w);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const float f = __uint_as_float(w[v]);
                if constexpr (MODE == QNN_POOL_MAX) mx[v] = fmaxf(mx[v], f);
                else sum[v] += (double)f;
            }
        }
    }
    const float fc = (float)((it.yb - it.ya) * (it.xb - it.xa));
    uint32_t out[V];
#pragma unroll
    for (int v = 0; v < V; ++v)
        out[v] = __float_as_uint(MODE == QNN_POOL_MAX ? mx[v] : __fdiv_rn((float)sum[v], fc));
    store_words<V>(reinterpret_cast<uint32_t*>(y + (size_t)it.q * p.cw + c0), out);
}

// Geometry of one call; QNN_EINVAL (with the error text set) for what qnn_abi_pool.h refuses.
int pool_geometry(const char* who, int H, int W, const qnn_pool2d_t* p, int* Ho, int* Wo, int* pt, int* pl) {
    QNN_REQUIRE(p, QNN_EINVAL, "%s: null descriptor", who);
    QNN_REQUIRE(p->mode == QNN_POOL_MAX || p->mode == QNN_POOL_AVG, QNN_EINVAL, "%s: mode=%d", who, p->mode);
    QNN_REQUIRE(p->same_pad == 0 || p->same_pad == 1, QNN_EINVAL, "%s: same_pad=%d", who, p->same_pad);
    QNN_REQUIRE(H > 0 && W > 0, QNN_EINVAL, "%s: image %dx%d", who, H, W);
    QNN_REQUIRE(p->ph > 0 && p->pw > 0 && p->sh > 0 && p->sw > 0, QNN_EINVAL, "%s: window %dx%d strides %dx%d", who, p->ph,
                p->pw, p->sh, p->sw);
    // (out - 1) * s + k stays far inside int: no window or stride beyond 2^15 is meaningful on an int image
    QNN_REQUIRE(p->ph <= 32768 && p->pw <= 32768 && p->sh <= 32768 && p->sw <= 32768 && H <= (1 << 24) && W <= (1 << 24),
                QNN_EINVAL, "%s: window %dx%d strides %dx%d image %dx%d out of range", who, p->ph, p->pw, p->sh, p->sw, H, W);
    QNN_REQUIRE(p->same_pad || (p->ph <= H && p->pw <= W), QNN_EINVAL,
                "%s: 'valid' window %dx%d is larger than the %dx%d image", who, p->ph, p->pw, H, W);
    qnn_same_pad(H, p->ph, p->sh, p->same_pad, Ho, pt);
    qnn_same_pad(W, p->pw, p->sw, p->same_pad, Wo, pl);
    // every window holds an in-bounds cell: the first and the last of each axis (the ones in between lie between them)
    const int ylast = (*Ho - 1) * p->sh - *pt, xlast = (*Wo - 1) * p->sw - *pl;
    QNN_REQUIRE(*Ho > 0 && *Wo > 0 && p->ph - *pt > 0 && p->pw - *pl > 0 && ylast < H && xlast < W && ylast + p->ph > 0 &&
                    xlast + p->pw > 0,
                QNN_EINVAL, "%s: a %dx%d window at strides %dx%d holds no cell of the %dx%d image", who, p->ph, p->pw,
                p->sh, p->sw, H, W);
    return QNN_OK;
}

template <int STORE>
void launch_packed(int mode, bool v4, const void* x, void* y, const PoolGeom& g, uint32_t total, float inv_m, hipStream_t s) {
    const dim3 grid((total + kBlock - 1) / kBlock), block(kBlock);
    const uint32_t* xu = (const uint32_t*)x;
    if (mode == QNN_POOL_MAX) {
        if (v4) hipLaunchKernelGGL((k_pool_max<STORE, 4>), grid, block, 0, s, xu, (uint32_t*)y, g, total);
        else hipLaunchKernelGGL((k_pool_max<STORE, 1>), grid, block, 0, s, xu, (uint32_t*)y, g, total);
    } else {
        // 32 sums per binary word: one word per lane keeps the register count of the other stores' four
        constexpr int V = STORE == QNN_STORE_BIN ? 1 : 4;
        if (v4) hipLaunchKernelGGL((k_pool_avg<STORE, V>), grid, block, 0, s, xu, (float*)y, g, total, inv_m);
        else hipLaunchKernelGGL((k_pool_avg<STORE, 1>), grid, block, 0, s, xu, (float*)y, g, total, inv_m);
    }
}

}  // namespace

extern "C" int qnn_pool2d_out_hw(int H, int W, const qnn_pool2d_t* p, int* Ho, int* Wo) {
    QNN_REQUIRE(Ho && Wo, QNN_EINVAL, "qnn_pool2d_out_hw: null pointer");
    int pt, pl;
    return pool_geometry("qnn_pool2d_out_hw", H, W, p, Ho, Wo, &pt, &pl);
}

extern "C" int qnn_pool2d_forward(const void* x, int x_store, int x_bits, int N, int H, int W, int C,
                                  const qnn_pool2d_t* p, void* y, int y_store, void* stream) {
    const char* who = "qnn_pool2d_forward";
    QNN_REQUIRE(x_store != QNN_STORE_T2, QNN_EUNSUPPORTED,
                "%s: no pooling on the ternary bit planes (QNN_STORE_T2): unpack, pool, pack", who);
    const bool packed = x_store == QNN_STORE_BIN || x_store == QNN_STORE_I4 || x_store == QNN_STORE_I8;
    QNN_REQUIRE(packed || x_store == QNN_STORE_F32, QNN_EINVAL, "%s: x_store=%d", who, x_store);
    QNN_REQUIRE(!(x_store == QNN_STORE_I4 || x_store == QNN_STORE_I8) || (x_bits >= 1 && x_bits <= x_store), QNN_EINVAL,
                "%s: x_bits=%d does not fit x_store=%d", who, x_bits, x_store);
    QNN_REQUIRE(N >= 0 && C > 0, QNN_EINVAL, "%s: shape (%d,%d,%d,%d)", who, N, H, W, C);
    PoolGeom g;
    int rc = pool_geometry(who, H, W, p, &g.Ho, &g.Wo, &g.pt, &g.pl);
    if (rc != QNN_OK) return rc;
    QNN_REQUIRE(y_store == (p->mode == QNN_POOL_MAX ? x_store : QNN_STORE_F32), QNN_EINVAL,
                "%s: y_store=%d (max: the input's store %d; avg: QNN_STORE_F32)", who, y_store, x_store);
    if (N == 0) return QNN_OK;
    QNN_REQUIRE(x && y, QNN_EINVAL, "%s: null pointer", who);
    g.H = H; g.W = W; g.C = C;
    g.ph = p->ph; g.pw = p->pw; g.sh = p->sh; g.sw = p->sw;
    g.cw = packed ? qnn_words(x_store, C) : C;
    const size_t xbytes = (size_t)N * H * W * g.cw * 4;
    const size_t ybytes = (size_t)N * g.Ho * g.Wo * (y_store == QNN_STORE_F32 ? (size_t)C : (size_t)g.cw) * 4;
    const uintptr_t xa = (uintptr_t)x, ya = (uintptr_t)y;
    QNN_REQUIRE(xa + xbytes <= ya || ya + ybytes <= xa, QNN_EINVAL, "%s: x and y overlap", who);
    // 16 bytes per lane where the words of a pixel divide by 4 (every pixel then starts 16-byte aligned)
    const bool v4 = g.cw % 4 == 0 && xa % 16 == 0 && ya % 16 == 0;
    const bool bin_avg = x_store == QNN_STORE_BIN && p->mode == QNN_POOL_AVG;
    g.groups = (v4 && !bin_avg) ? g.cw / 4 : g.cw;
    const size_t items = (size_t)N * g.Ho * g.Wo * g.groups;
    QNN_REQUIRE(items < ((size_t)1 << 31), QNN_EUNSUPPORTED, "%s: %zu work items (2^31 or more)", who, items);
    g.fd_g = qnn_fastdiv((uint32_t)g.groups);
    g.fd_wo = qnn_fastdiv((uint32_t)g.Wo);
    g.fd_ho = qnn_fastdiv((uint32_t)g.Ho);
    const uint32_t total = (uint32_t)items;
    hipStream_t s = (hipStream_t)stream;
    if (packed) {
        const float inv_m = x_store == QNN_STORE_BIN ? 1.0f : 1.0f / (float)(1u << (x_bits - 1));
        if (x_store == QNN_STORE_BIN) launch_packed<QNN_STORE_BIN>(p->mode, v4, x, y, g, total, inv_m, s);
        else if (x_store == QNN_STORE_I4) launch_packed<QNN_STORE_I4>(p->mode, v4, x, y, g, total, inv_m, s);
        else launch_packed<QNN_STORE_I8>(p->mode, v4, x, y, g, total, inv_m, s);
    } else {
        const dim3 grid((total + kBlock - 1) / kBlock), block(kBlock);
        const float* xf = (const float*)x;
        float* yf = (float*)y;
        if (p->mode == QNN_POOL_MAX) {
            if (v4) hipLaunchKernelGGL((k_pool_f32<QNN_POOL_MAX, 4>), grid, block, 0, s, xf, yf, g, total);
            else hipLaunchKernelGGL((k_pool_f32<QNN_POOL_MAX, 1>), grid, block, 0, s, xf, yf, g, total);
        } else {
            if (v4) hipLaunchKernelGGL((k_pool_f32<QNN_POOL_AVG, 4>), grid, block, 0, s, xf, yf, g, total);
            else hipLaunchKernelGGL((k_pool_f32<QNN_POOL_AVG, 1>), grid, block, 0, s, xf, yf, g, total);
        }
    }
    QNN_HIP(hipGetLastError());
    char name[32];
    snprintf(name, sizeof(name), "pool_%s_%s", p->mode == QNN_POOL_MAX ? "max" : "avg", store_name(x_store));
    qnn_set_kernel_name(name);
    return QNN_OK;
}
