// keras.layers.Cropping2D, UpSampling2D (nearest) and ZeroPadding2D on NHWC float32 tensors and on packed codes
// (include/qnn_abi_spatial.h).  Every output pixel is a copy of one input pixel or zero, and on the packed stores a pixel
// is a whole number of words: a word gather, no arithmetic, no bit funnel.  Between two low-bit layers the activation
// stays packed.
//
// Memory-bound, no reuse beyond the repeats: a repeated row or column re-reads lines that are still in cache.  One lane
// owns V consecutive 32-bit words (float32: channels) of one output pixel; consecutive lanes own consecutive groups of
// that pixel and then of the next pixel of the SAME output row, so loads and stores coalesce.  An output row is
// Wo * cw contiguous words of y, so item i of a row is stored at word i * V of it.
//
//   k_spatial<V, ROWS>   V = 4 (global_load_dwordx4 and one 16-byte store) where a pixel's word count divides by 4 and
//                        both pointers are 16-byte aligned, V = 1 otherwise.
//                        ROWS = false: one block per output row (blockIdx.x), the block strides along the row: the
//                        row's image, its source row and whether it is a zero row are block-uniform (scalar).
//                        ROWS = true: rows shorter than a block (a 16-pixel int4 row is 36 items): blockDim.x items by
//                        blockDim.y rows, one row per threadIdx.y; adjacent rows are adjacent in y, so a wave that
//                        spans two rows still stores one contiguous run.
// What depends on the row alone -- (n, oy), the division by up_y, the in-bounds test, the 64-bit row offsets -- is
// computed once in front of the loop along the row, never per word.  Zero rows and the zero columns at either end are
// stores only.  Row and pixel offsets are 64-bit, offsets inside a pixel and inside an output row 32-bit (the entry keeps
// the whole output below 2^31 words).  The mask of a pixel's last word comes from the host.
#include <stdio.h>

#include "qnn_common.h"
#include "qnn_abi_spatial.h"

namespace {

constexpr int kBlock = 256;

struct SpArgs {
    uint32_t rows;                     // N * Ho
    uint32_t row_items;                // Wo * groups
    uint32_t groups;                   // cw / V: items of one pixel
    uint32_t cw;                       // words of one pixel
    uint32_t last_mask;                // the real channels' bits of a pixel's last word (T2: of both words of its last pair)
    uint32_t tail;                     // words of a pixel the mask applies to: 1, T2: 2
    int32_t crop_t, crop_l, pad_t, pad_l;
    uint32_t live_h, live_w;           // Hc * up_y, Wc * up_x: the rows / columns that are copies
    uint64_t x_image, x_row;           // words of an input image, of an input row
    FastDiv fd_ho, fd_groups, fd_uy, fd_ux;
};

template <int V> struct Words;
template <> struct Words<1> {
    typedef uint32_t type;
    static __device__ __forceinline__ type zero() { return 0u; }
    static __device__ __forceinline__ void mask(type& v, uint32_t w0, const SpArgs& a) {
        if (w0 + a.tail >= a.cw) v &= a.last_mask;
    }
};
template <> struct Words<4> {
    typedef uint4 type;
    static __device__ __forceinline__ type zero() { return make_uint4(0u, 0u, 0u, 0u); }
    static __device__ __forceinline__ void mask(type& v, uint32_t w0, const SpArgs& a) {
        if (w0 + 4 >= a.cw) {
            v.w &= a.last_mask;
            if (a.tail == 2) v.z &= a.last_mask;
        }
    }
};

template <int V, bool ROWS>
__global__ __launch_bounds__(kBlock) void k_spatial(uint32_t* __restrict__ y, const uint32_t* __restrict__ x, const SpArgs a) {
    typedef Words<V> Wd;
    typedef typename Wd::type T;
    const uint32_t row = ROWS ? blockIdx.x * blockDim.y + threadIdx.y : blockIdx.x;
    if (row >= a.rows) return;
    // ---- per row ----
    const uint32_t n = qnn_div(row, a.fd_ho);
    const uint32_t oy = row - n * a.fd_ho.d;
    const uint32_t ly = oy - (uint32_t)a.pad_t;                        // wraps above live_h for the rows of the top pad
    const bool live = ly < a.live_h;
    const uint32_t* src = x;
    if (live) src += (size_t)n * a.x_image + (size_t)((uint32_t)a.crop_t + qnn_div(ly, a.fd_uy)) * a.x_row;
    uint32_t* dst = y + (size_t)row * a.row_items * V;
    // ---- along the row ----
    const uint32_t step = blockDim.x * gridDim.y;
    for (uint32_t i = blockIdx.y * blockDim.x + threadIdx.x; i < a.row_items; i += step) {
        T v = Wd::zero();
        if (live) {
            const uint32_t ox = qnn_div(i, a.fd_groups);
            const uint32_t w0 = (i - ox * a.groups) * V;
            const uint32_t lx = ox - (uint32_t)a.pad_l;
            if (lx < a.live_w) {
                const uint32_t sx = (uint32_t)a.crop_l + qnn_div(lx, a.fd_ux);
                v = *reinterpret_cast<const T*>(src + ((size_t)sx * a.cw + w0));
                Wd::mask(v, w0, a);
            }
        }
        *reinterpret_cast<T*>(dst + i * V) = v;
    }
}

int geometry(const char* who, int H, int W, const qnn_spatial2d_t* s, int64_t* Ho, int64_t* Wo) {
    QNN_REQUIRE(s, QNN_EINVAL, "%s: null descriptor", who);
    QNN_REQUIRE(H >= 1 && W >= 1, QNN_EINVAL, "%s: H=%d W=%d", who, H, W);
    for (int i = 0; i < 4; ++i) {
        QNN_REQUIRE(s->crop[i] >= 0, QNN_EINVAL, "%s: crop[%d]=%d is negative", who, i, s->crop[i]);
        QNN_REQUIRE(s->pad[i] >= 0, QNN_EINVAL, "%s: pad[%d]=%d is negative", who, i, s->pad[i]);
    }
    QNN_REQUIRE(s->up[0] >= 1 && s->up[1] >= 1, QNN_EINVAL, "%s: up=(%d, %d) (a repeat is at least 1)", who, s->up[0], s->up[1]);
    const int64_t Hc = (int64_t)H - s->crop[0] - s->crop[1], Wc = (int64_t)W - s->crop[2] - s->crop[3];
    QNN_REQUIRE(Hc >= 1 && Wc >= 1, QNN_EINVAL, "%s: crop ((%d, %d), (%d, %d)) leaves no %s of a %d x %d image", who,
                s->crop[0], s->crop[1], s->crop[2], s->crop[3], Hc < 1 ? "row" : "column", H, W);
    *Ho = Hc * s->up[0] + s->pad[0] + s->pad[1];
    *Wo = Wc * s->up[1] + s->pad[2] + s->pad[3];
    return QNN_OK;
}

}  // namespace

extern "C" int qnn_spatial2d_out_hw(int H, int W, const qnn_spatial2d_t* s, int* Ho, int* Wo) {
    const char* who = "qnn_spatial2d_out_hw";
    QNN_REQUIRE(Ho && Wo, QNN_EINVAL, "%s: null pointer", who);
    int64_t ho, wo;
    const int rc = geometry(who, H, W, s, &ho, &wo);
    if (rc != QNN_OK) return rc;
    QNN_REQUIRE(ho <= INT32_MAX && wo <= INT32_MAX, QNN_EUNSUPPORTED, "%s: a %lld x %lld output does not fit an int", who,
                (long long)ho, (long long)wo);
    *Ho = (int)ho;
    *Wo = (int)wo;
    return QNN_OK;
}

extern "C" int qnn_spatial2d_forward(const void* x, int store, int x_bits, int N, int H, int W, int C,
                                     const qnn_spatial2d_t* s, void* y, void* stream) {
    const char* who = "qnn_spatial2d_forward";
    int64_t Ho, Wo;
    const int rc = geometry(who, H, W, s, &Ho, &Wo);
    if (rc != QNN_OK) return rc;
    QNN_REQUIRE(N >= 0 && C >= 1, QNN_EINVAL, "%s: N=%d C=%d", who, N, C);
    const bool codes = store == QNN_STORE_I4 || store == QNN_STORE_I8;
    QNN_REQUIRE(codes || store == QNN_STORE_F32 || store == QNN_STORE_BIN || store == QNN_STORE_T2, QNN_EINVAL,
                "%s: store=%d", who, store);
    QNN_REQUIRE(!codes || (x_bits >= 1 && x_bits <= store), QNN_EINVAL, "%s: x_bits=%d does not fit store=%d", who, x_bits, store);
    const bool padded = s->pad[0] > 0 || s->pad[1] > 0 || s->pad[2] > 0 || s->pad[3] > 0;
    QNN_REQUIRE(!(store == QNN_STORE_BIN && padded), QNN_EUNSUPPORTED,
                "%s: zero padding on QNN_STORE_BIN: a +-1 code has no zero; unpack, pad in float32", who);
    const uint64_t cw = store == QNN_STORE_F32 ? (uint64_t)C : (uint64_t)qnn_words(store, C);
    const uint64_t lim = (uint64_t)1 << 31;
    QNN_REQUIRE((uint64_t)Ho < lim && (uint64_t)Wo < lim && (uint64_t)Ho * (uint64_t)Wo < lim &&
                (uint64_t)N * (uint64_t)Ho * (uint64_t)Wo < lim && (uint64_t)N * (uint64_t)Ho * (uint64_t)Wo * cw < lim,
                QNN_EUNSUPPORTED, "%s: %d x %lld x %lld pixels of %llu words (2^31 words or more)", who, N, (long long)Ho,
                (long long)Wo, (unsigned long long)cw);
    if (N == 0) return QNN_OK;
    QNN_REQUIRE(x && y, QNN_EINVAL, "%s: null pointer", who);
    const uintptr_t xa = (uintptr_t)x, ya = (uintptr_t)y;
    const uint64_t xbytes = (uint64_t)N * H * W * cw * 4, ybytes = (uint64_t)N * Ho * Wo * cw * 4;
    QNN_REQUIRE(xa + xbytes <= ya || ya + ybytes <= xa, QNN_EINVAL, "%s: y overlaps x", who);

    const int V = (cw % 4 == 0 && xa % 16 == 0 && ya % 16 == 0) ? 4 : 1;
    SpArgs a;
    a.rows = (uint32_t)((uint64_t)N * Ho);
    a.cw = (uint32_t)cw;
    a.groups = a.cw / V;
    a.row_items = (uint32_t)((uint64_t)Wo * a.groups);
    a.tail = store == QNN_STORE_T2 ? 2u : 1u;
    a.last_mask = ~0u;
    if (store != QNN_STORE_F32) {
        const int pw = store == QNN_STORE_T2 ? 32 : qnn_per_word(store), field = 32 / pw;
        const int used = (C - 1) % pw + 1;                             // channels of the last word
        if (used * field < 32) a.last_mask = (1u << (used * field)) - 1u;
    }
    a.crop_t = s->crop[0];
    a.crop_l = s->crop[2];
    a.pad_t = s->pad[0];
    a.pad_l = s->pad[2];
    a.live_h = (uint32_t)((int64_t)(H - s->crop[0] - s->crop[1]) * s->up[0]);
    a.live_w = (uint32_t)((int64_t)(W - s->crop[2] - s->crop[3]) * s->up[1]);
    a.x_row = (uint64_t)W * cw;
    a.x_image = (uint64_t)H * a.x_row;
    a.fd_ho = qnn_fastdiv((uint32_t)Ho);
    a.fd_groups = qnn_fastdiv(a.groups);
    a.fd_uy = qnn_fastdiv((uint32_t)s->up[0]);
    a.fd_ux = qnn_fastdiv((uint32_t)s->up[1]);

    hipStream_t st = (hipStream_t)stream;
    uint32_t* yu = (uint32_t*)y;
    const uint32_t* xu = (const uint32_t*)x;
    if (a.row_items * 2 <= (uint32_t)kBlock) {                         // at least two rows per block
        const uint32_t bx = a.row_items, by = (uint32_t)kBlock / bx;
        const dim3 grid((a.rows + by - 1) / by, 1), block(bx, by);
        if (V == 4) hipLaunchKernelGGL((k_spatial<4, true>), grid, block, 0, st, yu, xu, a);
        else hipLaunchKernelGGL((k_spatial<1, true>), grid, block, 0, st, yu, xu, a);
    } else {
        const uint32_t chunks = (a.row_items + kBlock - 1) / kBlock;
        const dim3 grid(a.rows, chunks < 65535u ? chunks : 65535u), block(kBlock);
        if (V == 4) hipLaunchKernelGGL((k_spatial<4, false>), grid, block, 0, st, yu, xu, a);
        else hipLaunchKernelGGL((k_spatial<1, false>), grid, block, 0, st, yu, xu, a);
    }
    QNN_HIP(hipGetLastError());
    qnn_set_kernel_name(store == QNN_STORE_F32 ? "spatial_f32" : store == QNN_STORE_BIN ? "spatial_bin" :
                        store == QNN_STORE_I4 ? "spatial_i4" : store == QNN_STORE_I8 ? "spatial_i8" : "spatial_t2");
    return QNN_OK;
}
