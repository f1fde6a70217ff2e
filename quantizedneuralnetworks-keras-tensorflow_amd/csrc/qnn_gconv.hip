// Keras Conv2D(groups = g) with float, binary, quantized or ternary weights (include/qnn_abi_gconv.h) on float32 tensors
// and on packed codes: filter f of group f / Fg reads the input channels [grp * Cg, (grp + 1) * Cg) only.  The integer
// arithmetic of the conv kernels and the shared float32 chain (qnn_epi_value / qnn_epi_code, qnn_common.h) behind it.
//
// k_gc_plain -- any window, stride, dilation, padding, store, group count: 32-bit (float32 input: float64) sums.
// qnn_pool.hip's lane map: one lane owns V consecutive 32-bit words (float32 output: V consecutive channels) of ONE output
// pixel, consecutive lanes own the next groups of that pixel and then of the next pixel.  V = 4 (16 bytes per lane) where
// the words per pixel divide by 4 and both pointers are 16-byte aligned, V = 1 otherwise.  It is the correctness form: per
// output channel and in-bounds tap it walks the words of the input pixel that hold the filter's group against the
// filter's words.  Those are prepacked in the input's word layout, `gw` words from the group's first word, with zero
// bits for every channel outside the group: a group edge may fall anywhere inside a word, and whatever x holds in its
// spare bits meets a zero weight (BIN: a mask over the group's bits).
//
// k_gc_mfma -- I4 / I8 codes in and out on v_mfma_i32_16x16x64_i8 for the shapes of qnn_gconv_plan.h.  A wave takes kPG
// groups of 16 output pixels (flattened over ONE image) x one TILE of 16 consecutive filters, which reads one contiguous
// run of R input channels.  The K = 64 of an MFMA is four slots of 16 channels, one per lane quad kq; the slots are the
// (tap, 16-channel chunk of the run) pairs, tap-major, so a 3x3 layer with R = 16 is 9 slots = 3 MFMAs.  Per K-step a lane
// loads its filter row's 16 bytes (A; prepacked per (tile, K-step) in operand order by k_gc_mfma_image, zero for padding
// slots and for the off-diagonal blocks of a multi-group tile) and, per pixel group, the 16 channels of ITS slot at its
// pixel (B; int4 widened to code * 16 bytes as the strip kernels do, the 1/16 folded into the output scale).  Which tap
// and chunk a (K-step, kq) holds is read from a table built at prepack (k_gc_slot_table): no division in the loop.  A tap
// outside the image, a pixel beyond the image and a padding slot are read through the image's buffer descriptor at an
// out-of-range offset: a zero operand, no branch.  A lane ends with the 4 consecutive filters 16 T + 4 kq .. + 3 of its
// pixel: one int8 word, stored as it is; for int4 half a word, so the lane quads kq and kq ^ 1 exchange halves of two
// pixel groups (one cross-lane move per pair of groups) and every lane stores one whole word.  No LDS, no scratch.
//
// Index arithmetic in 32 bits by multiply-high (the entry refuses 2^31 output words), tensor offsets in 64 bits.
#include <new>

#include "qnn_sideconv.h"
#include "qnn_strip_device.h"
#include "qnn_abi_gconv.h"
#include "qnn_gconv_plan.h"

struct qnn_gconv_weights : SideWeights {   // d_wq, d_wcode: [kh*kw][Cg][cout], Keras' (kh, kw, Cin / g, Cout) order
    int kh, kw, cin, cout, groups, Cg, Fg;
    int stride, same_pad, dil_h, dil_w;
    int gw;                  // words of an input pixel that one group can touch (the most over the groups)
    uint32_t* d_wpk;         // [kh*kw][cout][gw] the filter's codes in the word layout of an input pixel, or nullptr
    uint8_t* d_wm;           // matrix-pipe image [tile][K-step][lane 64][16 bytes], or nullptr
    int2* d_slots;           // matrix-pipe slot table [K-step][kq 4]: {dy | dx << 16, byte offset in the run or -1}
};

namespace {

constexpr int kBlock = 256;
constexpr int kPG = 4;       // 16-pixel groups a wave of k_gc_mfma takes per filter load (even: int4 pairs them)

// ---- weights ----------------------------------------------------------------------------------------------------------
// channels per word unit of a packed store and words per unit (T2: 32 channels in a (mask, sign) pair)
__host__ __device__ inline int gc_unit_channels(int store) { return store == QNN_STORE_T2 ? 32 : qnn_per_word(store); }
__host__ __device__ inline int gc_unit_words(int store) { return store == QNN_STORE_T2 ? 2 : 1; }
// first word of an input pixel that holds a channel of the group starting at channel clo
__host__ __device__ inline int gc_first_word(int store, int clo) { return clo / gc_unit_channels(store) * gc_unit_words(store); }

// word wi (of gw) of filter row (tap, f): the codes of the filter's group at the places the group's channels have in an
// input pixel on `store`, counted from the group's first word; every other field stays zero
__global__ __launch_bounds__(kBlock) void k_gc_pack_words(const int32_t* __restrict__ wcode, uint32_t* __restrict__ wpk,
                                                          int rows, int cout, int Cg, int Fg, int gw, int store) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= rows * gw) return;
    const int row = i / gw, wi = i - row * gw;
    const int tap = row / cout, f = row - tap * cout;
    const int clo = (f / Fg) * Cg;
    const int word0 = gc_first_word(store, clo) + wi;           // the word's index in the input pixel
    const int uc = gc_unit_channels(store), uw = gc_unit_words(store);
    const int c0 = word0 / uw * uc;                             // first channel of that word
    const int bits = store == QNN_STORE_T2 || store == QNN_STORE_BIN ? 1 : 32 / uc;
    const uint32_t mask = (1u << bits) - 1u;
    uint32_t word = 0;
    for (int j = 0; j < uc; ++j) {
        const int c = c0 + j - clo;                             // channel within the group
        if (c < 0 || c >= Cg) continue;
        const int code = wcode[((size_t)tap * Cg + c) * cout + f];
        uint32_t field;
        if (store == QNN_STORE_T2) field = (uint32_t)((word0 & 1) ? code > 0 : code != 0);
        else if (store == QNN_STORE_BIN) field = (uint32_t)(code > 0);
        else field = (uint32_t)code & mask;
        word |= field << (j * bits);
    }
    wpk[i] = word;
}

// One byte per thread of the image [tile][K-step][lane][16]: lane (r = lane & 15, kq = lane >> 4) of K-step k holds slot
// 4 k + kq = (tap, chunk) of filter 16 tile + r: the weight code (int8) at channel c0(tile) + 16 chunk +
// qnn_operand_channel(j) where that channel lies in the filter's group; zero elsewhere and in a padding slot.
__global__ __launch_bounds__(kBlock) void k_gc_mfma_image(const int32_t* __restrict__ wcode, uint8_t* __restrict__ wm,
                                                          const GcPlan p, int cout, int store, uint32_t total) {
    const uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (i >= total) return;
    uint32_t t = i;
    const int j = t & 15; t >>= 4;
    const int lane = t & 63; t >>= 6;
    const int step = (int)(t % (uint32_t)p.steps), tile = (int)(t / (uint32_t)p.steps);
    const int r = lane & 15, kq = lane >> 4;
    int tap, chunk, code = 0;
    if (qnn_gc_slot(&p, 4 * step + kq, &tap, &chunk)) {
        const int f = 16 * tile + r;
        const int c = qnn_gc_tile_channel(&p, tile) + 16 * chunk + qnn_operand_channel(store, j) - (f / p.Fg) * p.Cg;
        if (c >= 0 && c < p.Cg) code = wcode[((size_t)tap * p.Cg + c) * cout + f];
    }
    wm[i] = (uint8_t)(int8_t)code;
}

// entry (K-step, kq) of the slot table: the tap's row / column distance from the window's first cell and the chunk's
// byte offset in the tile's run; a padding slot has offset -1
__global__ __launch_bounds__(kBlock) void k_gc_slot_table(int2* __restrict__ tab, const GcPlan p, int kw, int dil_h, int dil_w,
                                                          int chunk_bytes) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= p.steps * 4) return;
    int tap, chunk;
    int2 v = make_int2(0, -1);
    if (qnn_gc_slot(&p, i, &tap, &chunk)) {
        const int ky = tap / kw, kx = tap - ky * kw;
        v = make_int2((ky * dil_h) | ((kx * dil_w) << 16), chunk * chunk_bytes);
    }
    tab[i] = v;
}

// ---- geometry ---------------------------------------------------------------------------------------------------------
struct GcGeom {
    int H, W, Ho, Wo, cin, cout, Cg, Fg;
    int kh, kw, stride, pt, pl, dil_h, dil_w;
    int xcw;                   // words (float32: channels) per input pixel
    int gw;                    // words per prepacked filter row
    int ocw;                   // words (float32: channels) per output pixel
    int groups;                // items per output pixel = ocw / V
    FastDiv fd_g, fd_wo, fd_ho, fd_fg;
};

// sum over the channels [clo, clo + Cg) of one packed pixel: `px` points at the group's first word (index w0 of the
// pixel), `wr` at the filter's nw words (zero outside the group)
template <int XS>
__device__ __forceinline__ int dot_group(const uint32_t* __restrict__ px, const uint32_t* __restrict__ wr, int nw, int w0,
                                         int clo, int chi, int acc) {
    if constexpr (XS == QNN_STORE_BIN) {
        // +-1 x +-1 over the group's bits of each word: n - 2 popcount((a ^ w) & valid)
        for (int wi = 0; wi < nw; ++wi) {
            const int cb = (w0 + wi) * 32;
            const int lo = max(clo, cb) - cb, hi = min(chi, cb + 32) - cb;
            if (hi <= lo) continue;
            const int nb = hi - lo;
            const uint32_t valid = (nb == 32 ? 0xFFFFFFFFu : (1u << nb) - 1u) << lo;
            acc += nb - 2 * __popc((px[wi] ^ wr[wi]) & valid);
        }
    } else if constexpr (XS == QNN_STORE_T2) {
        for (int wi = 0; wi < nw; wi += 2) acc = qnn_dot_t2(px[wi], px[wi + 1], wr[wi], wr[wi + 1], acc);
    } else {
        for (int wi = 0; wi < nw; ++wi) acc = qnn_dot<XS>(px[wi], wr[wi], acc);
    }
    return acc;
}

// ---- the plain form ---------------------------------------------------------------------------------------------------
// XS: the input's store.  The output's store is e.out_store (wave-uniform).  A lane walks its V output words, the
// channels of a word and the in-bounds taps of the pixel; a channel beyond cout - 1 is left out, so its bits stay zero.
template <int XS, int V>
__global__ __launch_bounds__(kBlock) void k_gc_plain(const void* __restrict__ x, const float* __restrict__ wq,
                                                     const uint32_t* __restrict__ wpk, void* __restrict__ y,
                                                     const GcGeom p, const EpiArgs e, const uint32_t total) {
    const uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (i >= total) return;
    const uint32_t q = qnn_div(i, p.fd_g);
    const int w0 = (int)(i - q * (uint32_t)p.groups) * V;
    const uint32_t tq = qnn_div(q, p.fd_wo);
    const int ox = (int)(q - tq * (uint32_t)p.Wo);
    const int n = (int)qnn_div(tq, p.fd_ho);
    const int oy = (int)(tq - (uint32_t)n * (uint32_t)p.Ho);
    const int iy0 = oy * p.stride - p.pt, ix0 = ox * p.stride - p.pl;
    const int opw = qnn_per_word(e.out_store), obits = 32 / opw;
    const uint32_t omask = obits == 32 ? 0xFFFFFFFFu : (1u << obits) - 1u;
    uint32_t out[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        uint32_t word = 0;
        for (int j = 0; j < opw; ++j) {
            const int oc = (w0 + v) * opw + j;
            if (oc >= p.cout) break;
            const int clo = (int)qnn_div((uint32_t)oc, p.fd_fg) * p.Cg;      // the group's first input channel
            int gw0 = 0, nw = 0;
            if constexpr (XS != QNN_STORE_F32) {
                gw0 = gc_first_word(XS, clo);
                nw = min(p.gw, p.xcw - gw0);
            }
            double facc = 0.0;
            int acc = 0;
            for (int ky = 0; ky < p.kh; ++ky) {
                const int iy = iy0 + ky * p.dil_h;
                if ((unsigned)iy >= (unsigned)p.H) continue;
                for (int kx = 0; kx < p.kw; ++kx) {
                    const int ix = ix0 + kx * p.dil_w;
                    if ((unsigned)ix >= (unsigned)p.W) continue;
                    const size_t pix = ((size_t)n * p.H + iy) * p.W + ix;
                    const int tap = ky * p.kw + kx;
                    if constexpr (XS == QNN_STORE_F32) {
                        const float* a = (const float*)x + pix * p.cin + clo;
                        const float* wr = wq + (size_t)tap * p.Cg * p.cout + oc;
                        for (int c = 0; c < p.Cg; ++c) facc += (double)a[c] * (double)wr[(size_t)c * p.cout];
                    } else {
                        acc = dot_group<XS>((const uint32_t*)x + pix * p.xcw + gw0,
                                            wpk + ((size_t)tap * p.cout + oc) * p.gw, nw, gw0, clo, clo + p.Cg, acc);
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
    store_words<V>((uint32_t*)y + (size_t)q * p.ocw + w0, out);
}

// ---- the matrix-pipe form -----------------------------------------------------------------------------------------------
struct GcMfma {
    int H, W, Ho, Wo;
    int stride, pt, pl;
    GcPlan plan;               // qnn_gconv_plan.h: K-steps per tile, 16-filter tiles, the tile's run
    int npix;                  // Ho * Wo
    int GT;                    // wave tasks per (image, tile): ceil(16-pixel groups / kPG)
    int pixb;                  // bytes per stored input pixel
    uint32_t img_bytes;        // one input image as stored
    uint32_t waves;            // N * GT * tiles
    FastDiv fd_tiles, fd_gt, fd_wo;
};

// XS = I4 / I8 (input and output store).  wave task = (image n, kPG groups from g0, tile), tile fastest: the waves that
// read the same pixels run next to each other.
template <int XS>
__global__ __launch_bounds__(kBlock) void k_gc_mfma(const uint8_t* __restrict__ x, const uint8_t* __restrict__ wm,
                                                    const int2* __restrict__ slots, uint32_t* __restrict__ y, const GcMfma p,
                                                    const EpiArgs e) {
    constexpr int LB = XS == QNN_STORE_I4 ? 8 : 16;       // bytes of a slot: 16 channels
    constexpr int OB = XS == QNN_STORE_I4 ? 4 : 8;
    const int lane = threadIdx.x & 63;
    const int r = lane & 15, kq = lane >> 4;
    const uint32_t wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)));
    if (wave >= p.waves) return;
    const uint32_t t1 = qnn_div(wave, p.fd_tiles);
    const int tile = (int)(wave - t1 * (uint32_t)p.plan.tiles);
    const int n = (int)qnn_div(t1, p.fd_gt);
    const int g0 = (int)(t1 - (uint32_t)n * (uint32_t)p.GT) * kPG;
    // byte offset of the tile's run inside a stored pixel (the run starts at a multiple of 16 channels)
    const int cbase = qnn_gc_tile_channel(&p.plan, tile) * OB / 8;

    // the lane's pixel of every group: the window's first cell (may lie outside the image) and the output pixel
    int by[kPG], bx[kPG];
    bool valid[kPG];
    uint32_t opix[kPG];
#pragma unroll
    for (int pg = 0; pg < kPG; ++pg) {
        const int pi = (g0 + pg) * 16 + r;
        valid[pg] = pi < p.npix;
        const int oy = (int)qnn_div((uint32_t)pi, p.fd_wo);
        const int ox = pi - oy * p.Wo;
        by[pg] = oy * p.stride - p.pt;
        bx[pg] = ox * p.stride - p.pl;
        opix[pg] = (uint32_t)n * (uint32_t)p.npix + (uint32_t)pi;
    }
    const __amdgpu_buffer_rsrc_t xr = strip_image_rsrc(x, n, p.img_bytes);
    const v4i* wt = reinterpret_cast<const v4i*>(wm) + (size_t)tile * p.plan.steps * 64 + lane;
    const int2* st = slots + kq;

    v4i acc[kPG];
#pragma unroll
    for (int pg = 0; pg < kPG; ++pg) acc[pg] = v4i{0, 0, 0, 0};

    for (int k = 0; k < p.plan.steps; ++k) {
        const v4i a = wt[(size_t)k * 64];
        const int2 sl = st[4 * k];
        const int dy = sl.x & 0xFFFF, dx = sl.x >> 16;
        v4i b[kPG];
#pragma unroll
        for (int pg = 0; pg < kPG; ++pg) {
            // a cell outside the image, a pixel beyond the image and a padding slot sit at an out-of-range offset: the
            // descriptor returns zeros
            const int iy = by[pg] + dy, ix = bx[pg] + dx;
            const bool ok = valid[pg] && sl.y >= 0 && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
            const int voff = ok ? (iy * p.W + ix) * p.pixb + cbase + sl.y : (int)0x80000000;
            if constexpr (XS == QNN_STORE_I4) {
                b[pg] = strip_widen(__builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(xr, voff, 0, 0)));
            } else {
                b[pg] = __builtin_bit_cast(v4i, __builtin_amdgcn_raw_buffer_load_b128(xr, voff, 0, 0));
            }
        }
#pragma unroll
        for (int pg = 0; pg < kPG; ++pg) acc[pg] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b[pg], acc[pg], 0, 0, 0);
    }

    // the lane's 4 consecutive filters: constants once, then the shared chain per value
    const int f0 = 16 * tile + 4 * kq;
    float cb[4], ci[4], cs[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
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
    uint32_t part[kPG];        // the 4 codes: a whole int8 word, half an int4 word
#pragma unroll
    for (int pg = 0; pg < kPG; ++pg) {
        uint32_t wd = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float val = qnn_epi_value(__fmul_rn((float)acc[pg][j], e.scale), j, le);
            wd |= ((uint32_t)qnn_epi_code(val, le) & MASK) << (OB * j);
        }
        part[pg] = wd;
    }
    if constexpr (XS == QNN_STORE_I8) {
#pragma unroll
        for (int pg = 0; pg < kPG; ++pg)
            if (valid[pg]) y[(size_t)opix[pg] * e.ocw + 4 * tile + kq] = part[pg];
    } else {
        // quads kq and kq ^ 1 hold the two halves of a word of the same pixel.  Per pair of groups (A, B) the even quad
        // hands over its half of B and receives the upper half of A, the odd quad the other way round: every lane ends
        // with one whole word -- the even quads of group A's pixel, the odd quads of group B's.
        const bool odd = (kq & 1) != 0;
#pragma unroll
        for (int pg = 0; pg < kPG; pg += 2) {
            const uint32_t recv = (uint32_t)__shfl_xor((int)(odd ? part[pg] : part[pg + 1]), 16, 64);
            const uint32_t word = odd ? (recv | (part[pg + 1] << 16)) : (part[pg] | (recv << 16));
            const bool ok = odd ? valid[pg + 1] : valid[pg];
            const uint32_t op = odd ? opix[pg + 1] : opix[pg];
            if (ok) y[(size_t)op * e.ocw + 2 * tile + (kq >> 1)] = word;
        }
    }
}

template <int XS>
void launch_plain(bool v4, const void* x, const qnn_gconv_weights* w, void* y, const GcGeom& g, const EpiArgs& e,
                  uint32_t total, hipStream_t s) {
    const dim3 grid((total + kBlock - 1) / kBlock), block(kBlock);
    if (v4) hipLaunchKernelGGL((k_gc_plain<XS, 4>), grid, block, 0, s, x, w->d_wq, w->d_wpk, y, g, e, total);
    else hipLaunchKernelGGL((k_gc_plain<XS, 1>), grid, block, 0, s, x, w->d_wq, w->d_wpk, y, g, e, total);
}

void out_hw(const qnn_gconv_weights* w, int H, int W, GcGeom* g) {
    qnn_same_pad_dilated(H, w->kh, w->stride, w->dil_h, w->same_pad, &g->Ho, &g->pt);
    qnn_same_pad_dilated(W, w->kw, w->stride, w->dil_w, w->same_pad, &g->Wo, &g->pl);
}

// prepack: the filter rows of the plain form on a packed store, and the operand image and slot table where the shape takes
// the matrix pipe
int pack_images(qnn_gconv_weights* w, hipStream_t s) {
    if (w->store != QNN_STORE_F32) {
        const int rows = w->kh * w->kw * w->cout, nw = rows * w->gw;      // below 2^31: checked with gw by the entry
        QNN_SIDE_HIP(hipMalloc(&w->d_wpk, (size_t)nw * sizeof(uint32_t)));
        hipLaunchKernelGGL(k_gc_pack_words, dim3((nw + kBlock - 1) / kBlock), dim3(kBlock), 0, s, w->d_wcode, w->d_wpk, rows,
                           w->cout, w->Cg, w->Fg, w->gw, w->store);
    }
    GcPlan plan;
    if (qnn_gc_mfma_ok(&plan, w->store, w->store, w->store, w->kh, w->kw, w->cin, w->cout, w->groups, 0, 0, 0)) {
        const size_t total = (size_t)plan.tiles * plan.steps * 64 * 16;      // below 2^31: qnn_gc_plan
        QNN_SIDE_HIP(hipMalloc(&w->d_wm, total));
        QNN_SIDE_HIP(hipMalloc(&w->d_slots, (size_t)plan.steps * 4 * sizeof(int2)));
        hipLaunchKernelGGL(k_gc_mfma_image, dim3((uint32_t)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, w->d_wcode,
                           w->d_wm, plan, w->cout, w->store, (uint32_t)total);
        hipLaunchKernelGGL(k_gc_slot_table, dim3((plan.steps * 4 + kBlock - 1) / kBlock), dim3(kBlock), 0, s, w->d_slots, plan,
                           w->kw, w->dil_h, w->dil_w, w->store == QNN_STORE_I4 ? 8 : 16);
    }
    return QNN_OK;
}

}  // namespace

extern "C" int qnn_gconv_prepack(int wkind, int wbits, float H, const float* kernel, int kh, int kw, int Cin, int Cout,
                                 int groups, const float* bias, int stride, int same_pad, int dil_h, int dil_w, int store,
                                 void* stream, qnn_gconv_weights_t** out) {
    const char* who = "qnn_gconv_prepack";
    QNN_REQUIRE(kernel && out, QNN_EINVAL, "%s: null pointer", who);
    QNN_REQUIRE(stride >= 1, QNN_EINVAL, "%s: stride=%d", who, stride);
    QNN_REQUIRE(dil_h >= 1 && dil_w >= 1, QNN_EINVAL, "%s: dilation=(%d,%d)", who, dil_h, dil_w);
    QNN_REQUIRE(kh > 0 && kw > 0 && Cin > 0 && Cout > 0, QNN_EINVAL, "%s: kernel shape (%d,%d) on %d -> %d channels", who, kh,
                kw, Cin, Cout);
    QNN_REQUIRE(groups >= 1, QNN_EINVAL, "%s: groups=%d", who, groups);
    QNN_REQUIRE(Cin % groups == 0 && Cout % groups == 0, QNN_EINVAL, "%s: groups=%d does not divide Cin=%d and Cout=%d", who,
                groups, Cin, Cout);
    QNN_REQUIRE(stride <= 2, QNN_EUNSUPPORTED, "%s: stride=%d (1 or 2)", who, stride);
    QNN_REQUIRE(kh <= QNN_GC_MAX_WINDOW, QNN_EUNSUPPORTED, "%s: kh=%d above QNN_GC_MAX_WINDOW = %d", who, kh, QNN_GC_MAX_WINDOW);
    QNN_REQUIRE(kw <= QNN_GC_MAX_WINDOW, QNN_EUNSUPPORTED, "%s: kw=%d above QNN_GC_MAX_WINDOW = %d", who, kw, QNN_GC_MAX_WINDOW);
    QNN_REQUIRE(dil_h <= QNN_MAX_DILATION && dil_w <= QNN_MAX_DILATION, QNN_EUNSUPPORTED,
                "%s: dilation=(%d,%d) above QNN_MAX_DILATION = %d", who, dil_h, dil_w, QNN_MAX_DILATION);
    QNN_REQUIRE((dil_h == 1 && dil_w == 1) || stride == 1, QNN_EUNSUPPORTED, "%s: dilation=(%d,%d) together with stride=%d",
                who, dil_h, dil_w, stride);
    const int Cg = Cin / groups, Fg = Cout / groups;
    QNN_REQUIRE((double)Cout * Cg * kh * kw < 1073741824.0, QNN_EUNSUPPORTED,
                "%s: the kernel has kh * kw * (Cin / groups) * Cout = %.0f values (2^30 or more)", who, (double)Cout * Cg * kh * kw);
    SideWeights common{};
    int rc = qnn_side_weights_check(who, wkind, wbits, H, store, &common);
    if (rc != QNN_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    qnn_gconv_weights* w = new (std::nothrow) qnn_gconv_weights();
    QNN_REQUIRE(w, QNN_ENOMEM, "%s: host allocation failed", who);
    *static_cast<SideWeights*>(w) = common;
    w->kh = kh; w->kw = kw; w->cin = Cin; w->cout = Cout; w->groups = groups; w->Cg = Cg; w->Fg = Fg;
    w->stride = stride; w->same_pad = same_pad ? 1 : 0;
    w->dil_h = dil_h; w->dil_w = dil_w;
    if (store != QNN_STORE_F32) {
        w->xcw = qnn_words(store, Cin);
        // the most words of a pixel one group touches: the span from its first channel's word to its last channel's
        const int uc = gc_unit_channels(store), uw = gc_unit_words(store);
        for (int grp = 0; grp < groups; ++grp) {
            const int span = (((grp + 1) * Cg - 1) / uc - grp * Cg / uc + 1) * uw;
            if (span > w->gw) w->gw = span;
        }
        const size_t row_words = (size_t)kh * kw * Cout * w->gw;
        if (row_words >= ((size_t)1 << 31)) {
            qnn_set_error("%s: the packed filter rows take kh * kw * Cout * %d = %zu words (2^31 or more)", who, w->gw, row_words);
            delete w;
            return QNN_EUNSUPPORTED;
        }
    }
    rc = qnn_side_quantize(w, kernel, kh * kw * Cg * Cout, bias, Cout, s);
    if (rc == QNN_OK) rc = pack_images(w, s);
    if (rc == QNN_OK) rc = qnn_side_hip(hipGetLastError(), "hipGetLastError()");
    if (rc != QNN_OK) {
        qnn_gconv_free(w);
        return rc;
    }
    *out = w;
    return QNN_OK;
}

extern "C" int qnn_gconv_free(qnn_gconv_weights_t* w) {
    if (!w) return QNN_OK;
    if (w->d_wpk) (void)hipFree(w->d_wpk);
    if (w->d_wm) (void)hipFree(w->d_wm);
    if (w->d_slots) (void)hipFree(w->d_slots);
    qnn_side_free(w);
    delete w;
    return QNN_OK;
}

extern "C" int qnn_gconv_dequant(const qnn_gconv_weights_t* w, float* kernel_khkwCF, void* stream) {
    QNN_REQUIRE(w && kernel_khkwCF, QNN_EINVAL, "qnn_gconv_dequant: null pointer");
    QNN_HIP(hipMemcpyAsync(kernel_khkwCF, w->d_wq, (size_t)w->kh * w->kw * w->Cg * w->cout * sizeof(float),
                           hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return QNN_OK;
}

extern "C" int qnn_gconv_out_hw(const qnn_gconv_weights_t* w, int H, int W, int* Ho, int* Wo) {
    QNN_REQUIRE(w && Ho && Wo, QNN_EINVAL, "qnn_gconv_out_hw: null pointer");
    QNN_REQUIRE(H > 0 && W > 0, QNN_EINVAL, "qnn_gconv_out_hw: image %dx%d", H, W);
    QNN_REQUIRE(H < (1 << 26) && W < (1 << 26), QNN_EINVAL, "qnn_gconv_out_hw: image %dx%d", H, W);
    GcGeom g;
    out_hw(w, H, W, &g);
    *Ho = g.Ho;
    *Wo = g.Wo;
    return QNN_OK;
}

extern "C" int qnn_gconv_forward(const qnn_gconv_weights_t* w, const void* x, int x_store, int x_bits, int N, int H, int W,
                                 const qnn_epilogue_t* epi, void* y, void* stream) {
    const char* who = "qnn_gconv_forward";
    QNN_REQUIRE(w && epi, QNN_EINVAL, "%s: null handle or epilogue", who);
    QNN_REQUIRE(N >= 0 && H > 0 && W > 0 && H < (1 << 26) && W < (1 << 26), QNN_EINVAL, "%s: N=%d H=%d W=%d", who, N, H, W);
    int xshift;
    EpiArgs e;
    int rc = qnn_side_forward_check(who, w, w->cout, x_store, x_bits, epi, "a grouped convolution", &xshift, &e);
    if (rc != QNN_OK) return rc;
    const bool packed = x_store != QNN_STORE_F32;
    // ---- the int32 bound: kh * kw * Cg (tap, channel) pairs, each at most 2^(x_bits-1) * 2^wshift ----
    if (packed) {
        const double worst = (double)w->kh * w->kw * w->Cg * (double)(1u << xshift) * (double)(1u << w->wshift);
        QNN_REQUIRE(worst < 2147483648.0, QNN_EUNSUPPORTED,
                    "%s: the int32 sum could overflow: kh * kw * Cg * 2^(x_bits-1) * 2^wshift = %.0f (2^31 or more)", who, worst);
    }
    // ---- geometry ----
    GcGeom g;
    out_hw(w, H, W, &g);
    QNN_REQUIRE(g.Ho > 0 && g.Wo > 0, QNN_EINVAL, "%s: empty output (%dx%d image, effective window %dx%d)", who, H, W,
                w->dil_h * (w->kh - 1) + 1, w->dil_w * (w->kw - 1) + 1);
    g.H = H; g.W = W; g.cin = w->cin; g.cout = w->cout; g.Cg = w->Cg; g.Fg = w->Fg;
    g.kh = w->kh; g.kw = w->kw; g.stride = w->stride; g.dil_h = w->dil_h; g.dil_w = w->dil_w;
    g.xcw = packed ? w->xcw : w->cin;
    g.gw = w->gw;
    g.ocw = e.ocw;
    bool run;
    rc = qnn_side_io_check(who, N, (size_t)N * g.Ho * g.Wo * (size_t)g.ocw, x, (size_t)N * H * W * g.xcw * 4, y, &run);
    if (!run) return rc;

    hipStream_t s = (hipStream_t)stream;
    GcPlan plan;
    const size_t img_bytes = (size_t)H * W * g.xcw * 4;
    const uintptr_t xa = (uintptr_t)x, ya = (uintptr_t)y;
    const bool fast = packed && w->d_wm && qnn_gc_mfma_ok(&plan, w->store, x_store, e.out_store, w->kh, w->kw, w->cin, w->cout,
                                                          w->groups, xa, ya, img_bytes);
    if (fast) {
        GcMfma p{};
        p.H = H; p.W = W; p.Ho = g.Ho; p.Wo = g.Wo;
        p.stride = w->stride; p.pt = g.pt; p.pl = g.pl;
        p.plan = plan;
        p.npix = g.Ho * g.Wo;                                                   // N * npix <= output words: below 2^31
        p.GT = ((p.npix + 15) / 16 + kPG - 1) / kPG;
        p.pixb = g.xcw * 4;
        p.img_bytes = (uint32_t)img_bytes;
        const size_t waves = (size_t)N * p.GT * plan.tiles;                        // <= output words: below 2^31
        p.waves = (uint32_t)waves;
        p.fd_tiles = qnn_fastdiv((uint32_t)plan.tiles);
        p.fd_gt = qnn_fastdiv((uint32_t)p.GT);
        p.fd_wo = qnn_fastdiv((uint32_t)g.Wo);
        if (x_store == QNN_STORE_I4) e.scale = ldexpf(e.scale, -4);              // operands are code * 16
        const dim3 grid((uint32_t)((waves + kBlock / 64 - 1) / (kBlock / 64))), block(kBlock);
        if (x_store == QNN_STORE_I4)
            hipLaunchKernelGGL((k_gc_mfma<QNN_STORE_I4>), grid, block, 0, s, (const uint8_t*)x, w->d_wm, w->d_slots,
                               (uint32_t*)y, p, e);
        else
            hipLaunchKernelGGL((k_gc_mfma<QNN_STORE_I8>), grid, block, 0, s, (const uint8_t*)x, w->d_wm, w->d_slots,
                               (uint32_t*)y, p, e);
    } else {
        const bool v4 = xa % 16 == 0 && ya % 16 == 0 && g.ocw % 4 == 0;
        g.groups = v4 ? g.ocw / 4 : g.ocw;
        g.fd_g = qnn_fastdiv((uint32_t)g.groups);
        g.fd_wo = qnn_fastdiv((uint32_t)g.Wo);
        g.fd_ho = qnn_fastdiv((uint32_t)g.Ho);
        g.fd_fg = qnn_fastdiv((uint32_t)g.Fg);
        const uint32_t total = (uint32_t)((size_t)N * g.Ho * g.Wo * (size_t)g.groups);
        qnn_side_for_store(x_store, [&](auto xs) { launch_plain<decltype(xs)::value>(v4, x, w, y, g, e, total, s); });
    }
    QNN_HIP(hipGetLastError());
    qnn_side_kernel_name("gconv", x_store, fast ? "_mfma" : "_plain");
    return QNN_OK;
}
