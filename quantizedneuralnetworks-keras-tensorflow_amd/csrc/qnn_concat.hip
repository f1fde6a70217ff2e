// keras.layers.Concatenate(axis=-1) on NHWC float32 tensors and on packed codes (include/qnn_abi_concat.h).  Between two
// low-bit layers the branches that meet are packed words, and their channel counts (growth rates such as 12 or 24) rarely
// fill whole words, so the packed form is a bit-funnel: the activation never exists in float32.
//
// Memory-bound, no reuse: every input word is read once (twice by the funnel where it straddles two output words: the
// second read hits L2).  One lane owns V consecutive 32-bit words (float32: channels) of ONE output pixel, consecutive
// lanes own consecutive groups of that pixel and then of the next pixel, as qnn_pool.hip.  One item per thread, index
// arithmetic in 32 bits by multiply-high (FastDiv): the entry refuses pixels * words >= 2^31; tensor offsets are 64-bit.
// The per-call table of the inputs is a kernel argument (SGPRs): the loops over it are unrolled over QNN_CONCAT_MAX with
// constant indices, so nothing is spilled to scratch and the only divergence is the word's own range test.
//
//   k_concat_words<V>    every input's width per pixel is a whole number of words (float32: always; packed: C_i * field a
//                        multiple of 32; T2: C_i a multiple of 32, the (mask, sign) pairs then concatenate as they are):
//                        each output group lies in exactly one input.  V = 4 (global_load_dwordx4 and one 16-byte store)
//                        where every width divides by 4 words and all pointers are 16-byte aligned, V = 1 otherwise.
//   k_concat_funnel<P>   any channel counts.  Output word w covers bits [32 w, 32 w + 32) of the pixel's concatenated bit
//                        string; for each input whose bit range meets it: the one or two source words that hold those
//                        bits, one funnel shift (v_alignbit_b32), AND with the mask of the bits that really are the
//                        input's channels, OR.  The mask makes the result independent of the inputs' spare bits.  P = 2
//                        runs the mask and the sign plane of QNN_STORE_T2 through the same steps.
#include <stdio.h>

#include "qnn_sideconv.h"
#include "qnn_abi_concat.h"

namespace {

constexpr int kBlock = 256;

struct CatArgs {
    const uint32_t* x[QNN_CONCAT_MAX];
    uint32_t beg[QNN_CONCAT_MAX];      // first word (k_concat_words) / first bit (k_concat_funnel) of input i in an output pixel
    uint32_t len[QNN_CONCAT_MAX];      // funnel: bits of input i per pixel (and plane)
    uint32_t cw[QNN_CONCAT_MAX];       // words of one pixel row of input i in memory
    int n;
    uint32_t items;                    // items per output pixel: word groups / funnel words (T2: word pairs)
    uint32_t ocw;                      // words of one pixel row of y
    uint32_t total;
    FastDiv fd;                        // by `items`
};

template <int V>
__global__ __launch_bounds__(kBlock) void k_concat_words(uint32_t* __restrict__ y, const CatArgs a) {
    const uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (i >= a.total) return;
    const uint32_t p = qnn_div(i, a.fd);
    const uint32_t w0 = (i - p * a.items) * V;
    // the input this group lies in: the last one that begins at or before it (the table is ascending)
    const uint32_t* src = a.x[0];
    uint32_t beg = 0, cw = a.cw[0];
#pragma unroll
    for (int k = 1; k < QNN_CONCAT_MAX; ++k)
        if (k < a.n && w0 >= a.beg[k]) {
            src = a.x[k];
            beg = a.beg[k];
            cw = a.cw[k];
        }
    typedef typename Words<V>::type T;
    const T v = *reinterpret_cast<const T*>(src + (size_t)p * cw + (w0 - beg));
    *reinterpret_cast<T*>(y + (size_t)p * a.ocw + w0) = v;
}

template <int PLANES>
__global__ __launch_bounds__(kBlock) void k_concat_funnel(uint32_t* __restrict__ y, const CatArgs a) {
    const uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (i >= a.total) return;
    const uint32_t p = qnn_div(i, a.fd);
    const uint32_t w = i - p * a.items;
    const int b0 = (int)(w * 32u);                     // the entry keeps a pixel below 2^31 bits
    uint32_t out[PLANES];
#pragma unroll
    for (int pl = 0; pl < PLANES; ++pl) out[pl] = 0u;
#pragma unroll
    for (int k = 0; k < QNN_CONCAT_MAX; ++k) {
        if (k < a.n) {
            const int len = (int)a.len[k];
            const int s = b0 - (int)a.beg[k];          // the source bit that lands on bit 0 of this word (< 0: the input begins inside it)
            if (s > -32 && s < len) {
                const int j = s >> 5;                  // source word of that bit; -1 where s < 0
                const uint32_t r = (uint32_t)s & 31u;  // = -beg mod 32: the same for every lane
                const int last = (len - 1) >> 5;
                const uint32_t* src = a.x[k] + (size_t)p * a.cw[k];
                const int lo_b = max(-s, 0), hi_b = min(len - s, 32);
                const uint32_t mask = (hi_b == 32 ? ~0u : (1u << hi_b) - 1u) & (~0u << lo_b);
#pragma unroll
                for (int pl = 0; pl < PLANES; ++pl) {
                    const uint32_t lo = j >= 0 ? src[PLANES * j + pl] : 0u;
                    const uint32_t hi = (r != 0u && j < last) ? src[PLANES * (j + 1) + pl] : 0u;
                    out[pl] |= __funnelshift_r(lo, hi, r) & mask;
                }
            }
        }
    }
    uint32_t* dst = y + (size_t)p * a.ocw + (size_t)PLANES * w;
#pragma unroll
    for (int pl = 0; pl < PLANES; ++pl) dst[pl] = out[pl];
}

}  // namespace

extern "C" int qnn_concat_forward(const qnn_concat_t* c, int store, int x_bits, size_t pixels, void* y, void* stream) {
    const char* who = "qnn_concat_forward";
    QNN_REQUIRE(c, QNN_EINVAL, "%s: null descriptor", who);
    const bool packed = store == QNN_STORE_BIN || store == QNN_STORE_I4 || store == QNN_STORE_I8;
    QNN_REQUIRE(packed || store == QNN_STORE_F32 || store == QNN_STORE_T2, QNN_EINVAL, "%s: store=%d", who, store);
    QNN_REQUIRE(!(store == QNN_STORE_I4 || store == QNN_STORE_I8) || (x_bits >= 1 && x_bits <= store), QNN_EINVAL,
                "%s: x_bits=%d does not fit store=%d", who, x_bits, store);
    QNN_REQUIRE(c->n >= 1 && c->n <= QNN_CONCAT_MAX, QNN_EINVAL, "%s: n=%d (1 .. %d inputs)", who, c->n, QNN_CONCAT_MAX);
    for (int i = 0; i < c->n; ++i)
        QNN_REQUIRE(c->channels[i] >= 1, QNN_EINVAL, "%s: channels[%d]=%d", who, i, c->channels[i]);
    // units per channel: bits of a packed field (T2: one bit in each of two planes), or one word for float32
    const int field = store == QNN_STORE_F32 ? 32 : store == QNN_STORE_T2 ? 1 : 32 / qnn_per_word(store);
    const int planes = store == QNN_STORE_T2 ? 2 : 1;
    uint64_t bits[QNN_CONCAT_MAX], sum = 0;
    bool whole = true;                                  // every input is a whole number of words per pixel (and plane)
    for (int i = 0; i < c->n; ++i) {
        bits[i] = (uint64_t)c->channels[i] * field;
        sum += bits[i];
        whole = whole && bits[i] % 32 == 0;
    }
    const uint64_t ocw = (sum + 31) / 32 * planes;      // words of an output pixel (float32: channels)
    QNN_REQUIRE(ocw < ((uint64_t)1 << 26), QNN_EUNSUPPORTED, "%s: %llu words per output pixel (2^26 or more)", who,
                (unsigned long long)ocw);
    QNN_REQUIRE(pixels < ((size_t)1 << 31) && (uint64_t)pixels * ocw < ((uint64_t)1 << 31), QNN_EUNSUPPORTED,
                "%s: %zu pixels of %llu words (2^31 words or more)", who, pixels, (unsigned long long)ocw);
    if (pixels == 0) return QNN_OK;
    QNN_REQUIRE(y, QNN_EINVAL, "%s: null pointer", who);
    const uintptr_t ya = (uintptr_t)y;
    const uint64_t ybytes = (uint64_t)pixels * ocw * 4;
    bool aligned = ya % 16 == 0;
    for (int i = 0; i < c->n; ++i) {
        QNN_REQUIRE(c->x[i], QNN_EINVAL, "%s: x[%d] is a null pointer", who, i);
        const uintptr_t xa = (uintptr_t)c->x[i];
        const uint64_t xbytes = (uint64_t)pixels * ((bits[i] + 31) / 32 * planes) * 4;
        QNN_REQUIRE(xa + xbytes <= ya || ya + ybytes <= xa, QNN_EINVAL, "%s: y overlaps x[%d]", who, i);
        aligned = aligned && xa % 16 == 0;
    }
    CatArgs a;
    a.n = c->n;
    a.ocw = (uint32_t)ocw;
    bool v4 = whole && aligned;
    uint64_t at = 0;
    for (int i = 0; i < QNN_CONCAT_MAX; ++i) {
        const bool in = i < c->n;
        a.x[i] = in ? (const uint32_t*)c->x[i] : nullptr;
        a.cw[i] = in ? (uint32_t)((bits[i] + 31) / 32 * planes) : 0u;
        a.len[i] = in ? (uint32_t)bits[i] : 0u;
        a.beg[i] = whole ? (uint32_t)(at / 32 * planes) : (uint32_t)at;      // words / bits in front of input i
        if (in) {
            at += bits[i];
            v4 = v4 && a.cw[i] % 4 == 0;
        }
    }
    const int V = v4 ? 4 : 1;
    a.items = whole ? a.ocw / V : a.ocw / planes;
    a.total = (uint32_t)(pixels * a.items);
    a.fd = qnn_fastdiv(a.items);
    const dim3 grid((a.total + kBlock - 1) / kBlock), block(kBlock);
    hipStream_t s = (hipStream_t)stream;
    uint32_t* yu = (uint32_t*)y;
    if (whole && v4) hipLaunchKernelGGL((k_concat_words<4>), grid, block, 0, s, yu, a);
    else if (whole) hipLaunchKernelGGL((k_concat_words<1>), grid, block, 0, s, yu, a);
    else if (planes == 2) hipLaunchKernelGGL((k_concat_funnel<2>), grid, block, 0, s, yu, a);
    else hipLaunchKernelGGL((k_concat_funnel<1>), grid, block, 0, s, yu, a);
    QNN_HIP(hipGetLastError());
    char name[16];
    snprintf(name, sizeof(name), "concat_%s", store_name(store));
    qnn_set_kernel_name(name);
    return QNN_OK;
}
