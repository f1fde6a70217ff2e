// 3x3 layers with int8-STORED activations and weights and 16 / 32 / 64 input channels (the 8-bit ResNets: full-qnn with
// wbits = 8 and / or abits = 8, models/resnet.py:104-129) as ROW-WALKING kernels on v_mfma_i32_16x16x64_i8: the int8
// form of qnn_mfma_strip.hip.  Dispatch: qnn_route_strip (qnn_route_strip.hip).
//
// The walk is the int4 one (see the header of qnn_mfma_strip.hip: a wave owns a 16-pixel-wide column strip of ONE image
// and walks down its rows; A = filters, B = pixels; one buffer descriptor per image so that SAME padding is an
// out-of-range load returning 0; a lane's C/D registers are 4 * NT consecutive channels of one pixel).  What differs:
//
//   * An int8 pixel already IS the B operand: 16 bytes per 16-channel k-block.  A lane fetches its k-block with ONE
//     16-byte load per K-step and input row and hands the register quad to the MFMA as it arrives -- there is no
//     widening and therefore no second register set: the ring of raw rows is the ring of operands.  R row slots hold
//     input rows yy - 1 .. yy + R - 3 when output row yy starts; the row's first instruction requests row yy + R - 2
//     into the slot row yy - 2 left, so R - 3 rows beyond the three being multiplied are in flight.
//   * The int8 weight codes in their natural [cout][tap][cin] order are the A image (qnn_mfma_prepare_weights points
//     d_mfma at d_packed).  Neither operand carries a factor 16: the scale is e.scale as it comes.
//   * A lane's 4 * NT channels are 4 * NT BYTES: one 4-byte (NT = 1) or 8-byte (NT = 2) store per row, and one shortcut
//     load of the same width.
//   * The epilogue is the float32 chain only (cvt, [bias], * inv, + shift, [shortcut FMA], round-half-even, clamp, each
//     operation rounded once; the file is built with -ffp-contract=off).  There is no fold: the accumulator domain
//     times 256 shortcut codes is far beyond what qnn_fold_prepare sweeps.  No projection inside the launch either: the
//     projection blocks keep the two-launch form (RES = 2, float32 shortcut).
//   * Rounding and clamping: as_int(u + 1.5 * 2^23) = 0x4B400000 + rint(u) for |u| < 2^22 and is monotone in u
//     everywhere, so a signed v_med3_i32 against 0x4B400000 - m and 0x4B400000 + m - 1 clamps it; the LOW BYTE of the
//     clamped word is the code in two's complement (0x4B400000 has a zero low byte), so four codes are gathered with
//     two v_perm_b32 and an OR, without the offset-code XOR of the nibble form.
//
// K order (as the int4 kernels): stride 1: k-block j = 4 * st + kq of an input row is (tap dx = j / BP, channel group
// j % BP), BP = Cin / 16; stride 2: lane group kq owns tap dx = kq and K-step st is channel group st.
//
// Register counts and waves per SIMD: the table below.
#include "qnn_mfma_common.h"
#include "qnn_strip_plan.h"
#include "qnn_strip_device.h"

// Waves per SIMD and ring slots, from the register counts of the ISA (unified 512-entry file per SIMD lane: 512 / waves,
// in steps of 8).  The ring costs 4 * ST registers per slot (twice the int4 kernel's raw ring), the filters 12 * ST * NT.
// VGPRs used (no bias .. bias; RES 0 / 1 / 2), no scratch in any instantiation:
//   Cin 16 (ST 1, NT 1): filters 12 + ring 24:  67-70 / 76-78 / 88-92     -> 6 waves (80 registers; RES 2: 5 waves, 96)
//   Cin 32 (ST 2, NT 2): filters 48 + ring 48:  144-152 / 160-168 / 184-192 -> 3 waves (168; RES 2: 2 waves, 256)
//   Cin 64 (ST 3, NT 2): filters 72 + ring 72:  194-204 / 212-216 / 232-240 -> 2 waves (256)
//   stride 2: Cin 16 94-102 -> 4 waves (128); Cin 32 134-150 -> 2 waves (the third would leave 18 spare registers)
#ifndef QNN_STRIP8_16_WPS
#define QNN_STRIP8_16_WPS 6
#endif
#ifndef QNN_STRIP8_32_WPS
#define QNN_STRIP8_32_WPS 3
#endif
#ifndef QNN_STRIP8_64_WPS
#define QNN_STRIP8_64_WPS 2
#endif
#ifndef QNN_STRIP8_SLOTS
#define QNN_STRIP8_SLOTS 6       // R: row slots of the operand ring (a multiple of 3: the float32 shortcut ring has 3)
#endif
// the float32 shortcut (RES = 2) adds a ring of 3 x NT x 4 registers: one wave per SIMD less where the budget is tight
constexpr int strip8_wps(int cin, int res) {
    return cin == 16 ? QNN_STRIP8_16_WPS - (res == 2 ? 1 : 0) : cin == 32 ? QNN_STRIP8_32_WPS - (res == 2 ? 1 : 0) : QNN_STRIP8_64_WPS;
}
#define QNN_STRIP8_S2_WPS(CIN) ((CIN) == 16 ? 4 : 2)   // stride 2: filters 24 / 48 + two row triples 24 / 48 + constants

namespace {

constexpr float kMagic8 = 12582912.0f;               // 1.5 * 2^23
constexpr int kMagic8Bits = 0x4B400000;

// Per-lane epilogue of both kernels: the lane's channels are nbase + 4 * NT * kq + 4 * nt + i.
// Everything behind the BN is scaled by powers of two only (activation code scale m, residual post-scale): those factors
// commute with every float32 rounding, so they are folded into the per-channel constants (qnn_mfma_strip.hip).
template <int NT, bool BIAS>
struct Strip8Epi {
    v2f nb[NT][2], ninv[NT][2], nshift[NT][2];
    v2f rcoef2, magic2;
    int code_lo, code_hi;
    bool binary;

    __device__ __forceinline__ void init(const EpiArgs& e, int c0, bool merge, bool packed_res) {
        binary = e.fn == QNN_FN_BINARY_TANH;
        const float cfold = (merge ? e.post_scale : 1.0f) * (binary ? 1.0f : e.act_m);
        const float rcoef = packed_res ? e.res_scale * cfold : cfold;   // shortcut code (or float value) -> scaled sum
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = c0 + 4 * nt + i;
                const float inv = e.bn_inv ? e.bn_inv[c] : 1.0f;
                const float shift = e.bn_inv ? e.bn_shift[c] : 0.0f;
                nb[nt][i >> 1][i & 1] = BIAS ? __fdiv_rn(e.bias[c], e.scale) : 0.0f;
                ninv[nt][i >> 1][i & 1] = __fmul_rn(__fmul_rn(inv, e.scale), cfold);
                nshift[nt][i >> 1][i & 1] = __fmul_rn(shift, cfold);
            }
        rcoef2 = v2f{rcoef, rcoef};
        magic2 = v2f{kMagic8, kMagic8};
        asm volatile("" : "+v"(magic2));             // a register pair (v_pk_add_f32 takes no literal): keeps the add packed
        code_lo = kMagic8Bits - (int)e.act_m;
        code_hi = kMagic8Bits + (int)e.act_m - 1;
    }

    // accumulators of tile nt -> its four bytes.  RES: 0 none, 1 packed int8 shortcut (the tile's word), 2 float32
    template <int RES>
    __device__ __forceinline__ uint32_t word(int nt, const v4i& acc, uint32_t rw, const float4& rf) const {
        v2f u2[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            v2f v = {(float)acc[2 * h], (float)acc[2 * h + 1]};   // |acc| <= 576 * 128 * 128 < 2^24: exact
            if constexpr (BIAS) v = v + nb[nt][h];
            v2f u = v * ninv[nt][h];                   // two roundings per value, as the reference's BN
            u = u + nshift[nt][h];
            if constexpr (RES == 1) {
                // shortcut value = code * 2^-(bits-1), exact: fma(code, scale, t) IS the reference's x + y
                const v2f cd = {(float)((int)(rw << (24 - 16 * h)) >> 24), (float)((int)(rw << (16 - 16 * h)) >> 24)};
                u = __builtin_elementwise_fma(cd, rcoef2, u);
            }
            if constexpr (RES == 2) {
                const v2f rv = h == 0 ? v2f{rf.x, rf.y} : v2f{rf.z, rf.w};
                u = __builtin_elementwise_fma(rv, rcoef2, u);   // (x + y) * 2^k == x*2^k + y*2^k, one rounding either way
            }
            u2[h] = u;
        }
        int cb[4];
        if (binary) {
            asm volatile("; binary_tanh codes");      // keeps this a real (uniform) branch
#pragma unroll
            for (int i = 0; i < 4; ++i) cb[i] = u2[i >> 1][i & 1] > 0x1p-24f ? kMagic8Bits + 1 : kMagic8Bits - 1;
        } else {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const v2f t = u2[h] + magic2;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int bits = __float_as_int(t[j]);
                    asm("v_med3_i32 %0, %1, %2, %3" : "=v"(cb[2 * h + j]) : "v"(bits), "v"(code_lo), "v"(code_hi));
                }
            }
        }
        // low byte of cb[i] = the code in two's complement
        const uint32_t lo = __builtin_amdgcn_perm((uint32_t)cb[1], (uint32_t)cb[0], 0x0C0C0400u);   // (c0, c1, 0, 0)
        const uint32_t hi = __builtin_amdgcn_perm((uint32_t)cb[3], (uint32_t)cb[2], 0x04000C0Cu);   // (0, 0, c2, c3)
        return lo | hi;
    }
};

template <int NT>
__device__ __forceinline__ void strip8_store(const uint32_t (&wd)[NT], __amdgpu_buffer_rsrc_t yr, int ovoff) {
    static_assert(NT == 1 || NT == 2, "a lane's bytes are one or two words");
    if constexpr (NT == 1) {
        __builtin_amdgcn_raw_buffer_store_b32(wd[0], yr, ovoff, 0, 0);
    } else {
        typedef uint32_t u2v __attribute__((ext_vector_type(2)));
        __builtin_amdgcn_raw_buffer_store_b64(u2v{wd[0], wd[1]}, yr, ovoff, 0, 0);
    }
}

// ---------------------------------------------------------------------------------------------------------
// stride 1.  RES: 0 none, 1 packed int8 shortcut (res_cw == ocw), 2 float32 shortcut
// ---------------------------------------------------------------------------------------------------------
template <int CIN, int NT, int RES, bool BIAS>
__global__ __launch_bounds__(256, strip8_wps(CIN, RES))
void k_conv_strip_i8(MfmaGeom mg, EpiArgs e, const uint8_t* __restrict__ x, const uint8_t* __restrict__ wq8,
                     void* __restrict__ y, int ntasks, int spr, FastDiv fd_spr, int nch, FastDiv fd_nch, int rc,
                     uint32_t img_x, uint32_t img_y, uint32_t img_r) {
    constexpr int BP = CIN / 16;                      // 16-channel k-blocks per pixel
    constexpr int ST = (3 * BP + 3) / 4;              // K-steps per input row: 1 / 2 / 3
    constexpr int PIXB = CIN;                         // bytes per stored input pixel
    constexpr int R = QNN_STRIP8_SLOTS;
    static_assert(R % 3 == 0 && R >= 6 && R <= 12, "ring slots: a multiple of three, 6 .. 12");
    const ConvGeom& g = mg.g;
    const int lane = threadIdx.x & 63;
    const int r = lane & 15, kq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int xw_, yb_;
    strip_block_map(xw_, yb_);
    const int wid = xw_ * 4 + wave, nw = gridDim.x * 4;
    const int nbase = yb_ * (16 * NT);                // first output channel of this wave

    // (deliberately NOT strip_kblocks / strip_load_filters of qnn_strip_device.h, which state the same table and load: through
    // them this kernel compiles differently, profiles/strip_chain/README.md.  Keep the two texts equal.)
    // ---- k-block of this lane in every K-step ----
    int dxs[ST], hbs[ST];
    bool kok[ST];
#pragma unroll
    for (int st = 0; st < ST; ++st) {
        const int j = 4 * st + kq;
        kok[st] = j < 3 * BP;
        dxs[st] = kok[st] ? j / BP : 1;
        hbs[st] = kok[st] ? j % BP : 0;
    }
    // ---- filters: A operand, row r of tile nt = channel nbase + 4*NT*(r>>2) + 4*nt + (r&3) (consecutive per lane in C/D) ----
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint8_t*>(wq8), 0, (int)mg.w_bytes, 0x00020000);
    v4i bw[3][ST][NT];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int st = 0; st < ST; ++st)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int ch = nbase + 4 * NT * (r >> 2) + 4 * nt + (r & 3);
                const int woff = kok[st] ? (ch * 9 + dy * 3 + dxs[st]) * CIN + hbs[st] * 16 : (int)0x80000000;
                bw[dy][st][nt] = __builtin_bit_cast(v4i, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, woff, 0, 0));
            }
    Strip8Epi<NT, BIAS> ep;
    ep.init(e, nbase + 4 * NT * kq, RES != 0, RES == 1);
    const int rowb = g.W * PIXB;                      // bytes per input row
    const int orowb = g.W * g.cout;                   // bytes per output row (ocw words = cout bytes per pixel)
    const int rrowb = RES == 2 ? g.W * g.cout * 4 : orowb;

    for (int task = wid; task < ntasks; task += nw) {
        const StripTask tk = strip_task(task, fd_nch, nch, fd_spr, spr, rc, g.H);
        const int n = tk.n, xs = tk.xs, y0 = tk.y0, y1 = tk.y1;
        const __amdgpu_buffer_rsrc_t xr = strip_image_rsrc(x, n, img_x), yr = strip_image_rsrc(y, n, img_y);
        const __amdgpu_buffer_rsrc_t rr = RES == 0 ? strip_image_rsrc(y, 0, 0) : strip_image_rsrc(e.res, n, img_r);
        // byte offset (inside the image) of this lane's k-block in input row y0 - 1; lanes whose pixel lies left or right of
        // the image start out of range and stay there (0x80000000 + row increments < 2^32); row -1 is a negative = huge
        // unsigned offset, the rows below the image end beyond the descriptor's size: both read as zeros
        int voff[ST];
#pragma unroll
        for (int st = 0; st < ST; ++st) {
            const int px = xs + r + dxs[st] - 1;
            voff[st] = (kok[st] && px >= 0 && px < g.W) ? ((y0 - 1) * g.W + px) * PIXB + hbs[st] * 16 : (int)0x80000000;
        }
        const bool pvalid = xs + r < g.W;                                       // last strip of a ragged row
        int ovoff = pvalid ? (y0 * g.W + xs + r) * g.cout + nbase + 4 * NT * kq : (int)0x80000000;   // 4*NT bytes
        int rvoff = RES == 2 ? (pvalid ? ((y0 * g.W + xs + r) * g.cout + nbase + 4 * NT * kq) * 4 : (int)0x80000000)
                             : ovoff;                                           // (f32: + 16 * nt, the next four floats)

        constexpr int RD = RES == 2 ? 3 : R;           // shortcut rows requested ahead (float32: 16 bytes per lane and tile)
        v4i ring[R][ST];
        uint32_t rs[RD][NT];
        float4 rf[RD][NT];
        auto load_row = [&](v4i (&dst)[ST]) {
#pragma unroll
            for (int st = 0; st < ST; ++st) {
                dst[st] = __builtin_bit_cast(v4i, __builtin_amdgcn_raw_buffer_load_b128(xr, voff[st], 0, 0));
                voff[st] += rowb;
            }
        };
        auto load_res = [&](uint32_t (&ds)[NT], float4 (&df)[NT]) {
            if constexpr (RES == 1) {
                if constexpr (NT == 1) {
                    ds[0] = __builtin_amdgcn_raw_buffer_load_b32(rr, rvoff, 0, 0);
                } else {
                    const uint2 t = __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(rr, rvoff, 0, 0));
                    ds[0] = t.x; ds[1] = t.y;
                }
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                if constexpr (RES == 2)
                    df[nt] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rr, rvoff + 16 * nt, 0, 0));
            rvoff += rrowb;
        };
#pragma unroll
        for (int d = 0; d < R - 1; ++d) load_row(ring[d]);                      // rows y0 - 1 .. y0 + R - 3
        if constexpr (RES != 0) {
#pragma unroll
            for (int d = 0; d < RD; ++d) load_res(rs[d], rf[d]);                // rows y0 .. y0 + RD - 1
        }

        // one output row yy = y0 + j: slots j, j+1, j+2 (mod R) hold input rows yy-1 / yy / yy+1; slot j-1 (row yy-2, done)
        // is refilled with row yy+R-2; shortcut slot j mod RD holds row yy (refilled with row yy+RD)
        auto body = [&](v4i (&Xa)[ST], v4i (&Xb)[ST], v4i (&Xc)[ST], v4i (&Xn)[ST], uint32_t (&rsc)[NT], float4 (&rfc)[NT]) {
            load_row(Xn);
            uint32_t rcur[NT];
            float4 fcur[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) { rcur[nt] = rsc[nt]; fcur[nt] = rfc[nt]; }
            if constexpr (RES != 0) load_res(rsc, rfc);
            v4i acc[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const v4i z = {0, 0, 0, 0};
                acc[nt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(bw[0][0][nt], Xa[0], z, 0, 0, 0);
#pragma unroll
                for (int st = 1; st < ST; ++st)
                    acc[nt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(bw[0][st][nt], Xa[st], acc[nt], 0, 0, 0);
#pragma unroll
                for (int st = 0; st < ST; ++st)
                    acc[nt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(bw[1][st][nt], Xb[st], acc[nt], 0, 0, 0);
#pragma unroll
                for (int st = 0; st < ST; ++st)
                    acc[nt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(bw[2][st][nt], Xc[st], acc[nt], 0, 0, 0);
            }
            uint32_t wd[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) wd[nt] = ep.template word<RES>(nt, acc[nt], rcur[nt], fcur[nt]);
            strip8_store<NT>(wd, yr, ovoff);
            ovoff += orowb;
        };
#define STRIP8_BODY(J) body(ring[(J) % R], ring[((J) + 1) % R], ring[((J) + 2) % R], ring[((J) + R - 1) % R], rs[(J) % RD], rf[(J) % RD])
        int yy = y0;
        for (; yy + R <= y1; yy += R) {
            STRIP8_BODY(0); STRIP8_BODY(1); STRIP8_BODY(2); STRIP8_BODY(3); STRIP8_BODY(4); STRIP8_BODY(5);
            if constexpr (R > 6) { STRIP8_BODY(6); STRIP8_BODY(7); STRIP8_BODY(8); }
            if constexpr (R > 9) { STRIP8_BODY(9); STRIP8_BODY(10); STRIP8_BODY(11); }
        }
        const int rem = y1 - yy;
        if (rem > 0) STRIP8_BODY(0);
        if (rem > 1) STRIP8_BODY(1);
        if (rem > 2) STRIP8_BODY(2);
        if (rem > 3) STRIP8_BODY(3);
        if (rem > 4) STRIP8_BODY(4);
        if constexpr (R > 6) { if (rem > 5) STRIP8_BODY(5); if (rem > 6) STRIP8_BODY(6); if (rem > 7) STRIP8_BODY(7); }
        if constexpr (R > 9) { if (rem > 8) STRIP8_BODY(8); if (rem > 9) STRIP8_BODY(9); if (rem > 10) STRIP8_BODY(10); }
#undef STRIP8_BODY
    }
}

// ---------------------------------------------------------------------------------------------------------
// stride 2 (the first conv of a stage; no residual merge behind it): the walk over OUTPUT rows of k_conv_strip_s2
// (qnn_mfma_strip.hip).  Lane group kq owns tap dx = kq and fetches its whole input pixel 2*(xs + r) - pl + kq with
// CIN / 16 sixteen-byte loads per input row; every output row requests its three input rows one output row ahead.
// ---------------------------------------------------------------------------------------------------------
template <int CIN, int NT, bool BIAS>
__global__ __launch_bounds__(256, QNN_STRIP8_S2_WPS(CIN))
void k_conv_strip_i8_s2(MfmaGeom mg, EpiArgs e, const uint8_t* __restrict__ x, const uint8_t* __restrict__ wq8,
                        void* __restrict__ y, int ntasks, int spr, FastDiv fd_spr, int nch, FastDiv fd_nch, int rc,
                        uint32_t img_x, uint32_t img_y) {
    constexpr int ST = CIN / 16;                       // K-step st = channel group st of tap kq
    constexpr int PIXB = CIN;
    const ConvGeom& g = mg.g;                          // g.H, g.W: input; g.Ho, g.Wo: output
    const int lane = threadIdx.x & 63;
    const int r = lane & 15, kq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int xw_, yb_;
    strip_block_map(xw_, yb_);
    const int wid = xw_ * 4 + wave, nw = gridDim.x * 4;
    const int nbase = yb_ * (16 * NT);
    int dxs[ST], hbs[ST];
    bool kok[ST];
    strip_kblocks_s2(kq, dxs, hbs, kok);
    v4i bw[3][ST][NT];                                 // as in k_conv_strip_i8
    strip_load_filters<CIN>(bw, wq8, mg.w_bytes, nbase, r, kok, dxs, hbs);
    Strip8Epi<NT, BIAS> ep;
    ep.init(e, nbase + 4 * NT * kq, false, false);
    const int rowb2 = 2 * g.W * PIXB;                  // two input rows per output row
    const int orowb = g.Wo * g.cout;
    for (int task = wid; task < ntasks; task += nw) {
        const StripTask tk = strip_task(task, fd_nch, nch, fd_spr, spr, rc, g.Ho);
        const int n = tk.n, xs = tk.xs, y0 = tk.y0, y1 = tk.y1;
        const __amdgpu_buffer_rsrc_t xr = strip_image_rsrc(x, n, img_x), yr = strip_image_rsrc(y, n, img_y);
        int voff[3];
        const int px = 2 * (xs + r) - g.pl + kq;
        const bool pvalid = xs + r < g.Wo;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
            voff[dy] = (kq < 3 && px >= 0 && px < g.W && pvalid) ? ((2 * y0 - g.pt + dy) * g.W + px) * PIXB : (int)0x80000000;
        int ovoff = pvalid ? (y0 * g.Wo + xs + r) * g.cout + nbase + 4 * NT * kq : (int)0x80000000;
        v4i raw[2][3][ST];
        auto load_rows = [&](v4i (&dst)[3][ST]) {
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
#pragma unroll
                for (int st = 0; st < ST; ++st)
                    dst[dy][st] = __builtin_bit_cast(v4i, __builtin_amdgcn_raw_buffer_load_b128(xr, voff[dy] + 16 * st, 0, 0));
                voff[dy] += rowb2;
            }
        };
        load_rows(raw[0]);
        auto body = [&](v4i (&cur)[3][ST], v4i (&nxt)[3][ST]) {
            load_rows(nxt);                            // the three input rows of the next output row
            v4i acc[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[nt] = v4i{0, 0, 0, 0};
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int st = 0; st < ST; ++st)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
                        acc[nt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(bw[dy][st][nt], cur[dy][st], acc[nt], 0, 0, 0);
            uint32_t wd[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) wd[nt] = ep.template word<0>(nt, acc[nt], 0u, float4{});
            strip8_store<NT>(wd, yr, ovoff);
            ovoff += orowb;
        };
        int yy = y0;
        for (; yy + 2 <= y1; yy += 2) {
            body(raw[0], raw[1]);
            body(raw[1], raw[0]);
        }
        if (yy < y1) body(raw[0], raw[1]);
    }
}

template <int CIN, int NT>
int launch_strip8_s2(const MfmaGeom& mg, const EpiArgs& e, const void* x, const uint8_t* w, void* y, hipStream_t s) {
    const ConvGeom& g = mg.g;
    const int spr = (g.Wo + 15) / 16;
    const int ny = g.cout / (16 * NT);
    const double img_x = (double)g.H * g.W * CIN, img_y = (double)g.Ho * g.Wo * g.cout;
    if (img_x >= 1.0e9 || img_y >= 1.0e9 || ny < 1 || ny * 16 * NT != g.cout) return 1;
    const int wps = QNN_STRIP8_S2_WPS(CIN);
    StripPlan p;                // over output rows, as the int4 stride-2 form
    if (!qnn_strip_plan(&p, g.N, spr, g.Ho, 256 * wps / ny > 0 ? 256 * wps / ny : 1, 2, 1)) return 1;
    const dim3 grid(p.blocks, (unsigned)ny), block(256);
    if (e.bias)
        hipLaunchKernelGGL((k_conv_strip_i8_s2<CIN, NT, true>), grid, block, 0, s, mg, e, (const uint8_t*)x, w, y,
                           QNN_STRIP_PLAN_ARGS(p), (uint32_t)img_x, (uint32_t)img_y);
    else
        hipLaunchKernelGGL((k_conv_strip_i8_s2<CIN, NT, false>), grid, block, 0, s, mg, e, (const uint8_t*)x, w, y,
                           QNN_STRIP_PLAN_ARGS(p), (uint32_t)img_x, (uint32_t)img_y);
    return 0;
}

template <int CIN, int NT>
int launch_strip8(const MfmaGeom& mg, const EpiArgs& e, const void* x, const uint8_t* w, void* y, hipStream_t s) {
    const ConvGeom& g = mg.g;
    const int spr = (g.W + 15) / 16;
    const int ny = g.cout / (16 * NT);
    const double img_x = (double)g.H * g.W * CIN, img_y = (double)g.H * g.W * g.cout;
    const int res = !e.res ? 0 : e.res_store == QNN_STORE_F32 ? 2 : 1;
    const double img_r = res == 2 ? img_y * 4.0 : img_y;
    if (img_x >= 1.0e9 || img_y >= 1.0e9 || img_r >= 1.0e9 || ny < 1 || ny * 16 * NT != g.cout) return 1;
    const int wps = strip8_wps(CIN, res);
    StripPlan p;                // fill 3: taken over from the int4 walk with its value (stale there, see launch_strip)
    if (!qnn_strip_plan(&p, g.N, spr, g.H, 256 * wps / ny > 0 ? 256 * wps / ny : 1, 3, 1)) return 1;
    const dim3 grid(p.blocks, (unsigned)ny), block(256);
    const bool bias = e.bias != nullptr;
#define STRIP8_CASE(RES_, BIAS_)                                                                                  \
    if (res == RES_ && bias == BIAS_) {                                                                           \
        hipLaunchKernelGGL((k_conv_strip_i8<CIN, NT, RES_, BIAS_>), grid, block, 0, s, mg, e, (const uint8_t*)x, w, y, \
                           QNN_STRIP_PLAN_ARGS(p), (uint32_t)img_x, (uint32_t)img_y, (uint32_t)img_r);            \
        return 0;                                                                                                 \
    }
    STRIP8_CASE(0, false) STRIP8_CASE(0, true) STRIP8_CASE(1, false) STRIP8_CASE(1, true)
    STRIP8_CASE(2, false) STRIP8_CASE(2, true)
#undef STRIP8_CASE
    return 1;
}

}  // namespace

// cin in {16, 32, 64} (stride 2: 16, 32), cout a multiple of 16 / 32 / 32; eligibility is checked by the caller
int qnn_launch_strip_i8(int cin, const MfmaGeom& mg, const EpiArgs& e, const void* x, const uint8_t* w,
                        void* y, hipStream_t s) {
    if (mg.g.stride == 2) {
        if (e.res) return 1;
        return cin == 16 ? launch_strip8_s2<16, 2>(mg, e, x, w, y, s) : cin == 32 ? launch_strip8_s2<32, 2>(mg, e, x, w, y, s) : 1;
    }
    if (cin == 16) return launch_strip8<16, 1>(mg, e, x, w, y, s);
    if (cin == 32) return launch_strip8<32, 2>(mg, e, x, w, y, s);
    if (cin == 64) return launch_strip8<64, 2>(mg, e, x, w, y, s);
    return 1;
}
