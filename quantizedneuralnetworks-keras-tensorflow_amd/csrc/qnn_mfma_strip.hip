// 3x3 stride-1 int4 layers with 16 or 32 channels (the 224x224 and 112x112 stages of the ImageNet ResNet,
// models/resnet.py:104-129) as a ROW-WALKING kernel on v_mfma_i32_16x16x64_i8.
// Dispatch: qnn_route_strip (qnn_mfma.hip).  The same layers with int8-STORED activations and weights (the 8-bit
// ResNets) run on the int8 form of this walk, qnn_mfma_strip_i8.hip: no widening, 16-byte operand loads, byte epilogue.
//
// These layers are bound by instruction issue, not by the matrix pipe (16 x 16 outputs need 3 or 12 MFMAs of 16
// cycles) and not by HBM: QuantizedConv2D.call (quantized_layers.py:164-194) + BN + residual merge + quantized_tanh
// is ~11 float32 VALU operations per output value whatever the kernel does.  So everything else is removed:
//
//   * A wave owns a 16-pixel-wide column strip of ONE image and walks down its rows.  The widened operands of an
//     input row are built once and used by the three output rows that need it (register rotation, loop unrolled by
//     three): per output row one 8-byte load per lane and K-step instead of nine per tile.
//   * Operand roles are swapped: A = filters (rows = output channels), B = pixels (columns).  In the C/D layout a
//     lane then holds FOUR CONSECUTIVE CHANNELS OF ONE PIXEL -- 16 bits of the packed output word: the lane stores
//     them with one 2-byte store (64 lanes = one full 128-byte line) and fetches its shortcut codes with one 2-byte
//     load.  No nibble transposes, no cross-lane traffic at all.
//   * Zero padding costs nothing inside the loop: every tensor is addressed through a buffer descriptor of ONE image,
//     so the rows above the first and below the last are out of range (raw buffer loads return 0); the left / right
//     edge lanes of the first / last strip get an out-of-range offset once per strip.  No masks, no scalar decode per
//     tile (the previous kernel spent ~88 scalar and ~84 vector instructions per 16 pixels; this one ~50 vector).
//
// K order: an input row contributes 3*BP sixteen-channel k-blocks (BP = Cin/16 blocks per pixel), block j = (tap
// dx = j / BP, channel group j % BP); K-step st (64 deep = four k-blocks) takes j = 4*st + kq:
//   Cin 16: one step, kq = dx (kq = 3: zero filter);  Cin 32: (dx0 lo, dx0 hi, dx1 lo, dx1 hi), (dx2 lo, dx2 hi, 0, 0);
//   Cin 64: one step per tap.  int4 codes are widened to code*16 in both operands (x256 folded into the power-of-two
//   output scale), exactly as in qnn_mfma_small.hip.
// (Round 3 measured the other cut -- lane group kq owns tap dx = kq and fetches its whole pixel with 16-byte loads, BP
// K-steps three quarters full -- on the stride-1 kernel: Cin 32 unchanged (18.7 / 16.4 us), Cin 64 slower (16.6 against
// 14.8 us: a fourth K-step and 30 more registers); the stride-2 kernel below keeps it, 14.0 -> 12.2 us at Cin 32.)
// Filter rows are dealt to the NT channel tiles so that a lane's 4*NT results are CONSECUTIVE channels (tile nt, row
// 4*kq + i  <->  channel nbase + 4*NT*kq + 4*nt + i): with NT = 2 the two 16-bit fields of a lane are one 32-bit word,
// i.e. ONE store and ONE shortcut load per row instead of two each (round 3: the 32- and 64-channel layers ran with the
// texture-address FIFOs full, SQ_VMEM_TA_ADDR_FIFO_FULL 2.4-2.9 M against 0.3 M on the 16-channel layers).
// A wave computes 16*NT output channels (blockIdx.y selects the block): Cin 64 -> 64 runs as two 32-channel halves so
// that the 18 filter fragments stay in registers.  Any width: the last strip of a row is partly out of the image (its
// loads and stores get out-of-range offsets).
#include "qnn_mfma_common.h"
#include "qnn_fold.h"
#include "qnn_strip_plan.h"
#include "qnn_strip_device.h"

#ifndef QNN_STRIP16_WPS
#define QNN_STRIP16_WPS 6        // waves per SIMD (= persistent workgroups per CU): Cin 16 needs 51-67 VGPRs
#endif
#ifndef QNN_STRIP32_WPS
#define QNN_STRIP32_WPS 1        // Cin 32: 118-128 VGPRs.  Round 4: ONE wave per SIMD with a six-row ring (3 before): same layer time,
                                 // room for the other batches' kernels: ResNet-224 with three batches in flight 85.1 -> 87.0 K img/s
#endif
#ifndef QNN_STRIP64_WPS
#define QNN_STRIP64_WPS 1        // Cin 64 (two 32-channel halves per strip): 164-200 VGPRs, spills at 3 per SIMD.  Round 4: ONE
                                 // wave per SIMD with a six-row ring: the layer alone is as fast as with two (11.3 / 13.2 us),
                                 // and the other batch's kernels find room beside it: ResNet-224 end to end 77.4 -> 79.5 K img/s
#endif
#ifndef QNN_STRIP16_DEPTH
#define QNN_STRIP16_DEPTH 3      // input rows requested ahead of the row being computed (see the ring in k_conv_strip)
#endif
#ifndef QNN_STRIP32_DEPTH
#define QNN_STRIP32_DEPTH 6
#endif
#ifndef QNN_STRIP64_DEPTH
#define QNN_STRIP64_DEPTH 6
#endif

namespace {

// FN: the activation of the un-folded epilogue as a template parameter.  0 = quantized_tanh or binary_tanh (told apart at
// run time, as ever: these instantiations are instruction for instruction what they were), QNN_FN_QUANTIZED_RELU,
// QNN_FN_QUANTIZED_LEAKYRELU (qnn_common.h: qnn_qact_code_f is what k_conv_generic evaluates; here in code units, u = v * m):
//   quantized_relu       t = u + m, ONE more packed add per channel pair: m is a power of two, so this is fadd_rn(v, 1) * m
//                        exactly, the contract's only rounding.  Then the magic add with the offset lowered by m:
//                        as_int(t + (1.5 * 2^23 + 8 - m)) = 0x4B400008 + rint(t) - m (the offset stays even, so ties still
//                        go to even), and the integer clamp to [0, m - 1].
//   quantized_leakyrelu  u = max(u, 0.1f * u): one packed multiply per pair and one v_max_f32 per value.  Equal to the
//                        contract's select for every u that is not NaN: u >= 0 gives 0.1f * u <= u (both zeros for u = +-0),
//                        u < 0 gives |0.1f * u| <= |u| hence 0.1f * u >= u; 0.1f * (u = v * m) = (0.1f * v) * m exactly.
//                        tests/test_qrelu_cpu.py holds this form against the reference's vectors.
template <int FN>
__device__ __forceinline__ void strip_qact(v2f (&u2)[2], const v2f& m2, const v2f& alpha2) {
    static_assert(FN == 0 || FN == QNN_FN_QUANTIZED_RELU || FN == QNN_FN_QUANTIZED_LEAKYRELU, "activation of the strip epilogue");
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if constexpr (FN == QNN_FN_QUANTIZED_RELU) u2[h] = u2[h] + m2;
        if constexpr (FN == QNN_FN_QUANTIZED_LEAKYRELU) {
            const v2f s = u2[h] * alpha2;
            u2[h] = v2f{fmaxf(u2[h][0], s[0]), fmaxf(u2[h][1], s[1])};
        }
    }
}

// FOLD: the epilogue as integer thresholds (qnn_fold.h; e.fold_a / e.fold_b, proven equal to the float32 chain on the
// layer's whole accumulator domain by qnn_fold_prepare): the offset is the MFMA's initial accumulator, then per value
// cvt + mul, per pair one v_cvt_pknorm_i16_f32 (+ two v_pk_add_i16 clamp with a shortcut), and the nibbles of a lane's
// field are gathered with two v_perm_b32 + shift + v_bfi_b32 (NT = 2) instead of cvt, [add], mul, add, [bfe, cvt, fma],
// add, v_med3 and a shift-or per value.
// RES: 0 none, 1 packed int4 shortcut, 2 float32 shortcut, 3 projection shortcut computed here (qnn_projection_t: the
// 1x1 strides-2 convolution of the block input with CIN / 2 channels, one more MFMA per tile and row on the even pixels of
// the even input rows -- the float32 tensor RES = 2 reads is never formed); FOLD: 0 chain, 1 / 2 = fold modes (qnn_fold.h)
template <int CIN, int NT, int RES, bool BIAS, int FOLD, int FN = 0>
__global__ __launch_bounds__(256, (CIN == 16 ? QNN_STRIP16_WPS : CIN == 32 ? (RES == 2 ? 2 : QNN_STRIP32_WPS) : QNN_STRIP64_WPS)) void k_conv_strip(MfmaGeom mg, EpiArgs e,
                                                                 const uint8_t* __restrict__ x,
                                                                 const uint8_t* __restrict__ wq8,
                                                                 void* __restrict__ y, int ntasks, int spr,
                                                                 FastDiv fd_spr, int nch, FastDiv fd_nch, int rc,
                                                                 uint32_t img_x, uint32_t img_y, uint32_t img_r) {
    constexpr int BP = CIN / 16;                      // 16-channel k-blocks per pixel
    constexpr int ST = (3 * BP + 3) / 4;              // K-steps per input row: 1 / 2 / 3
    constexpr int PIXB = CIN / 2;                     // bytes per stored input pixel
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
    // ---- filters: A operand, row = output channel nt*16 + r ----
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint8_t*>(wq8), 0, (int)mg.w_bytes, 0x00020000);
    v4i bw[3][ST][NT];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int st = 0; st < ST; ++st)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int ch = nbase + 4 * NT * (r >> 2) + 4 * nt + (r & 3);       // filter of A row r in tile nt
                const int woff = kok[st] ? (ch * 9 + dy * 3 + dxs[st]) * CIN + hbs[st] * 16 : (int)0x80000000;
                bw[dy][st][nt] = __builtin_bit_cast(v4i, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, woff, 0, 0));
            }
    // ---- epilogue constants: this lane's channels are nbase + 4*NT*kq + 4*nt + i ----
    // Everything behind the BN is scaled by powers of two only (activation code scale m, residual post-scale): those
    // factors commute with every float32 rounding, so they are folded into the per-channel constants and the epilogue
    // is cvt, [add bias], mul, add, [fma shortcut], round, clamp per value.
    const bool binary = e.fn == QNN_FN_BINARY_TANH;
    const float cfold = (RES != 0 ? e.post_scale : 1.0f) * (binary ? 1.0f : e.act_m);
    const float rcoef = RES == 1 ? e.res_scale * cfold : cfold;        // shortcut code (or float value) -> scaled sum
    // (the float32 steps run on channel PAIRS: v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32 round each half exactly like
    // their scalar forms and issue at the same rate -- tools/micro/pk_f32_rate.hip -- so the multiply, the two adds and
    // the shortcut FMA cost half an instruction per value)
    v2f nb[NT][2], ninv[NT][2], nshift[NT][2];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = nbase + 4 * NT * kq + 4 * nt + i;
            const float inv = e.bn_inv ? e.bn_inv[c] : 1.0f;
            const float shift = e.bn_inv ? e.bn_shift[c] : 0.0f;
            nb[nt][i >> 1][i & 1] = BIAS ? __fdiv_rn(e.bias[c], e.scale) : 0.0f;
            ninv[nt][i >> 1][i & 1] = __fmul_rn(__fmul_rn(inv, e.scale), cfold);
            nshift[nt][i >> 1][i & 1] = __fmul_rn(shift, cfold);
        }
    const v2f rcoef2 = {rcoef, rcoef};
    // folded epilogue: per-channel slope and accumulator offset (the MFMA chain starts from the offset)
    static_assert(!FOLD || RES < 2, "the float32 shortcuts are not folded");
    static_assert(!FOLD || FN == 0, "only quantized_tanh is folded");
    static_assert(RES != 3 || (NT == 2 && CIN >= 32), "projection shortcut: 32 / 64 channel stages");
    // ---- projection shortcut (RES = 3): 1x1 filters as one more A operand per tile; K-blocks beyond CIN / 2 channels are
    // out of range = zeros, and so are the same lanes' pixel loads ----
    constexpr int P0B = CIN / 4;                      // bytes per stored pixel of the block input (CIN / 2 channels)
    constexpr int BPP = CIN / 32;                     // its 16-channel k-blocks: 1 / 2
    v4i bwp[NT];
    v2f pbias[NT][2];
    const v2f pscale2 = {e.proj_scale, e.proj_scale};
    if constexpr (RES == 3) {
        const __amdgpu_buffer_rsrc_t prsrc = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<uint8_t*>(e.proj_w), 0, g.cout * (CIN / 2), 0x00020000);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int ch = nbase + 4 * NT * (r >> 2) + 4 * nt + (r & 3);
            const int woff = kq < BPP ? ch * (CIN / 2) + kq * 16 : (int)0x80000000;
            bwp[nt] = __builtin_bit_cast(v4i, __builtin_amdgcn_raw_buffer_load_b128(prsrc, woff, 0, 0));
#pragma unroll
            for (int i = 0; i < 4; ++i)
                pbias[nt][i >> 1][i & 1] = e.proj_bias ? e.proj_bias[nbase + 4 * NT * kq + 4 * nt + i] : 0.0f;
        }
    }
    const bool has_pbias = e.proj_bias != nullptr;
    float fa[NT][4], fc[NT][4];
    v4i binit[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = nbase + 4 * NT * kq + 4 * nt + i;
            fa[nt][i] = FOLD ? e.fold_a[c] : 0.0f;
            fc[nt][i] = FOLD == 2 ? e.fold_c[c] : 0.0f;
            binit[nt][i] = FOLD ? e.fold_b[c] : 0;
        }
    // round-half-even + clamp + offset code in the integer domain: as_int(u + (1.5*2^23 + 8)) = 0x4B400008 + rint(u)
    // for |u| < 2^22 and is monotone in u everywhere, so a signed integer med3 clamps it; the low nibble is code + 8
    constexpr float kMagic = 12582920.0f;
    constexpr int kMagicBits = 0x4B400008;
    const float mgc = FN == QNN_FN_QUANTIZED_RELU ? kMagic - e.act_m : kMagic;     // (an even integer either way: act_bits >= 2)
    v2f magic2 = {mgc, mgc};
    asm volatile("" : "+v"(magic2));                  // a register pair (v_pk_add_f32 takes no literal): keeps the add packed
    const int code_lo = FN == QNN_FN_QUANTIZED_RELU ? kMagicBits : kMagicBits - (int)e.act_m, code_hi = kMagicBits + (int)e.act_m - 1;
    const v2f act_m2 = {e.act_m, e.act_m}, alpha2 = {0.1f, 0.1f};      // strip_qact<FN>; unused for FN = 0
    const int rowb = g.W * PIXB;                      // bytes per input row
    const int orowb = g.W * e.ocw * 4;                // bytes per output row
    const int rrowb = RES == 2 ? g.W * g.cout * 4 : RES == 3 ? 2 * e.proj_W * P0B : orowb;   // (RES = 3: every other input row)

    for (int task = wid; task < ntasks; task += nw) {
        const StripTask tk = strip_task(task, fd_nch, nch, fd_spr, spr, rc, g.H);
        const int n = tk.n, xs = tk.xs, y0 = tk.y0, y1 = tk.y1;
        const __amdgpu_buffer_rsrc_t xr = strip_image_rsrc(x, n, img_x), yr = strip_image_rsrc(y, n, img_y);
        const __amdgpu_buffer_rsrc_t rr = RES == 0 ? strip_image_rsrc(y, 0, 0)           // (never read)
                                                   : strip_image_rsrc(RES == 3 ? (const void*)e.proj_x : e.res, n, img_r);
        // byte offset (inside the image) of this lane's k-block in input row y0 - 1; lanes whose pixel lies left or right of
        // the image start out of range and stay there (0x80000000 + row increments < 2^32)
        int voff[ST];
#pragma unroll
        for (int st = 0; st < ST; ++st) {
            const int px = xs + r + dxs[st] - 1;
            voff[st] = (kok[st] && px >= 0 && px < g.W) ? ((y0 - 1) * g.W + px) * PIXB + hbs[st] * 8 : (int)0x80000000;
        }
        const bool pvalid = xs + r < g.W;                                       // last strip of a ragged row
        int ovoff = pvalid ? (y0 * g.W + xs + r) * e.ocw * 4 + nbase / 2 + kq * 2 * NT : (int)0x80000000;   // 2*NT bytes
        int rvoff = RES == 2 ? (pvalid ? ((y0 * g.W + xs + r) * g.cout + nbase + 4 * NT * kq) * 4 : (int)0x80000000)
                    : RES == 3 ? ((pvalid && kq < BPP) ? (2 * y0 * e.proj_W + 2 * (xs + r)) * P0B + kq * 8 : (int)0x80000000)
                             : ovoff;                                           // + nt*16 (f32: the next four floats)

        // Loads are requested D rows ahead (a ring of D raw input-row register sets and D shortcut registers): vmcnt retires
        // in issue order, so a wave that waits for the oldest request keeps D - 1 rows of younger ones in flight.  Round 4:
        // with the folded epilogue the kernels are no longer bound by instruction issue but by the bytes they keep in
        // flight (6144 waves x 3 rows x 128 unique bytes = 2.4 MB against ~1 us of loaded HBM latency = the 2.4 TB/s they
        // reached): the ring depth is a compile-time constant per channel count (QNN_STRIP*_DEPTH, a multiple of 3).
        constexpr int D = RES == 2 ? 3          // (the float32 shortcut of a projection block: 16 bytes per lane, row and tile)
                          : CIN == 16 ? QNN_STRIP16_DEPTH : CIN == 32 ? QNN_STRIP32_DEPTH : QNN_STRIP64_DEPTH;
        static_assert(D % 3 == 0 && D >= 3, "the row loop is unrolled D times and rotates three operand sets");
        v4i X[3][ST];
        uint2 raw[D][ST];
        uint32_t rs[D][NT];                            // packed shortcut: [.][0] holds the lane's whole 2*NT-byte field
        float4 rf[D][NT];
        auto load_row = [&](uint2 (&dst)[ST]) {
#pragma unroll
            for (int st = 0; st < ST; ++st) {
                dst[st] = __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(xr, voff[st], 0, 0));
                voff[st] += rowb;
            }
        };
        auto load_res = [&](uint32_t (&ds)[NT], float4 (&df)[NT]) {
            if constexpr (RES == 1) {
                if constexpr (NT == 1) ds[0] = __builtin_amdgcn_raw_buffer_load_b16(rr, rvoff, 0, 0);
                else ds[0] = __builtin_amdgcn_raw_buffer_load_b32(rr, rvoff, 0, 0);        // both tiles' codes in one word
            }
            if constexpr (RES == 3) {                  // this lane's k-block of block-input pixel (2 yy, 2 (xs + r)): 16 codes
                const uint2 t = __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(rr, rvoff, 0, 0));
                ds[0] = t.x; ds[NT - 1] = t.y;
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                if constexpr (RES == 2)
                    df[nt] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rr, rvoff + 16 * nt, 0, 0));
            rvoff += rrowb;
        };
        {
            uint2 t0[ST], t1[ST];
            load_row(t0);                              // row y0 - 1
            load_row(t1);                              // row y0
#pragma unroll
            for (int d = 0; d < D; ++d) load_row(raw[d]);                       // rows y0 + 1 .. y0 + D
            if constexpr (RES != 0) {
#pragma unroll
                for (int d = 0; d < D; ++d) load_res(rs[d], rf[d]);             // rows y0 .. y0 + D - 1
            }
#pragma unroll
            for (int st = 0; st < ST; ++st) X[0][st] = strip_widen(t0[st]);
#pragma unroll
            for (int st = 0; st < ST; ++st) X[1][st] = strip_widen(t1[st]);
        }

        // one output row yy = y0 + j: X slots a / b / c = j, j+1, j+2 (mod 3) hold input rows yy-1 / yy / yy+1; ring slot
        // j mod D holds row yy+1 (consumed here, refilled with row yy+1+D); shortcut slot j mod D holds row yy (refilled
        // with row yy+D)
        auto body = [&](v4i (&Xa)[ST], v4i (&Xb)[ST], v4i (&Xc)[ST], uint2 (&rw)[ST], uint32_t (&rsc)[NT],
                        float4 (&rfc)[NT]) {
#pragma unroll
            for (int st = 0; st < ST; ++st) Xc[st] = strip_widen(rw[st]);
            load_row(rw);                              // row yy + 1 + D
            uint32_t rcur[NT];
            float4 fcur[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) { rcur[nt] = rsc[nt]; fcur[nt] = rfc[nt]; }
            if constexpr (RES != 0) load_res(rsc, rfc);   // shortcut of row yy + D
            v4i accp[NT];
            if constexpr (RES == 3) {
                const v4i Xp = strip_widen(make_uint2(rcur[0], rcur[NT - 1]));
                const v4i z0 = {0, 0, 0, 0};
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) accp[nt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(bwp[nt], Xp, z0, 0, 0, 0);
            }
            v4i acc[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const v4i z = binit[nt];               // zeros, or the fold's per-channel offsets
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
            if constexpr (FOLD) {
                // ---- folded epilogue (qnn_fold.h) ----
                if constexpr (NT == 1) {
                    // pairs (c0, c2), (c1, c3): codes in bits 12-15 / 28-31 of a pair
                    uint32_t pe = qnn_fold_pair_m<FOLD>(acc[0][0], acc[0][2], fa[0][0], fa[0][2], fc[0][0], fc[0][2]);
                    uint32_t po = qnn_fold_pair_m<FOLD>(acc[0][1], acc[0][3], fa[0][1], fa[0][3], fc[0][1], fc[0][3]);
                    if constexpr (RES == 1) {
                        // shortcut field (16 bits): nibbles -> offset codes (sc + 8) << 10 in the halves of a pair
                        const uint32_t w = rcur[0] ^ 0x8888u;
                        const uint32_t yy2 = __builtin_amdgcn_perm(0u, w, 0x0C010C00u);          // bytes (b0, 0, b1, 0)
                        pe = qnn_fold_merge(pe, (yy2 & 0x000F000Fu) << 10);
                        po = qnn_fold_merge(po, (yy2 & 0x00F000F0u) << 6);
                    }
                    const uint32_t mm = (po & 0xF000F000u) | ((pe >> 4) & ~0xF000F000u);          // v_bfi_b32: bytes 1, 3 = (c1:c0), (c3:c2)
                    const uint32_t o16 = __builtin_amdgcn_perm(0u, mm, 0x0C0C0301u);
                    __builtin_amdgcn_raw_buffer_store_b16((unsigned short)o16, yr, ovoff, 0, 0);
                } else {
                    static_assert(NT <= 2, "a lane's fields must fit one word");
                    uint32_t tp[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        tp[j] = qnn_fold_pair_m<FOLD>(acc[0][j], acc[1][j], fa[0][j], fa[1][j], fc[0][j], fc[1][j]);   // (c_j, c_j+4)
                    if constexpr (RES == 1) {
                        const uint32_t w = rcur[0] ^ 0x88888888u;
                        tp[0] = qnn_fold_merge(tp[0], (w & 0x000F000Fu) << 10);
                        tp[1] = qnn_fold_merge(tp[1], (w & 0x00F000F0u) << 6);
                        tp[2] = qnn_fold_merge(tp[2], (w & 0x0F000F00u) << 2);
                        tp[3] = qnn_fold_merge(tp[3], (w & 0xF000F000u) >> 2);
                    }
                    const uint32_t uo = __builtin_amdgcn_perm(tp[3], tp[1], 0x07030501u);         // (c1, c3, c5, c7) in the high nibbles
                    const uint32_t ue = __builtin_amdgcn_perm(tp[2], tp[0], 0x07030501u);         // (c0, c2, c4, c6)
                    const uint32_t o32 = (uo & 0xF0F0F0F0u) | ((ue >> 4) & 0x0F0F0F0Fu);
                    __builtin_amdgcn_raw_buffer_store_b32(o32, yr, ovoff, 0, 0);
                }
                ovoff += orowb;
                return;
            }
            // ---- epilogue: the reference's op order, one rounding per operation ----
            uint32_t field[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                v2f u2[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    v2f v = {(float)acc[nt][2 * h], (float)acc[nt][2 * h + 1]};
                    if constexpr (BIAS) v = v + nb[nt][h];
                    v2f u = v * ninv[nt][h];                       // two roundings per value, as the reference's BN
                    u = u + nshift[nt][h];
                    if constexpr (RES == 1) {
                        // shortcut value = code * 2^-(bits-1), exact: fma(code, scale, t) IS the reference's x + y
                        const v2f cd = {(float)((int)(rcur[0] << (28 - 8 * h - 16 * nt)) >> 28),
                                        (float)((int)(rcur[0] << (24 - 8 * h - 16 * nt)) >> 28)};
                        u = __builtin_elementwise_fma(cd, rcoef2, u);
                    }
                    if constexpr (RES == 2) {
                        const v2f rv = h == 0 ? v2f{fcur[nt].x, fcur[nt].y} : v2f{fcur[nt].z, fcur[nt].w};
                        u = __builtin_elementwise_fma(rv, rcoef2, u);   // (x + y) * 2^k == x*2^k + y*2^k, one rounding either way
                    }
                    if constexpr (RES == 3) {
                        // the float32 value k_conv_pw_f32 stores for this shortcut: float(sum) * scale [+ bias], one rounding each
                        v2f rv = v2f{(float)accp[nt][2 * h], (float)accp[nt][2 * h + 1]} * pscale2;
                        if (has_pbias) rv = rv + pbias[nt][h];
                        u = __builtin_elementwise_fma(rv, rcoef2, u);
                    }
                    u2[h] = u;
                }
                int cb[4];
                strip_qact<FN>(u2, act_m2, alpha2);
                if (FN == 0 && binary) {
                    asm volatile("; binary_tanh codes");          // keeps this a real (uniform) branch
#pragma unroll
                    for (int i = 0; i < 4; ++i) cb[i] = u2[i >> 1][i & 1] > 0x1p-24f ? kMagicBits + 1 : kMagicBits - 1;
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
                // low nibble of cb[i] = code + 8, bits 4..21 are zero: three shift-ors assemble the 16-bit field
                uint32_t P = ((uint32_t)cb[1] << 4) | (uint32_t)cb[0];
                P = ((uint32_t)cb[2] << 8) | P;
                P = ((uint32_t)cb[3] << 12) | P;
                field[nt] = P;                             // bits 16.. hold shifted bits of the magic constant
            }
            if constexpr (NT == 1) {
                __builtin_amdgcn_raw_buffer_store_b16((unsigned short)(field[0] ^ 0x8888u), yr, ovoff, 0, 0);
            } else {
                static_assert(NT <= 2, "a lane's fields must fit one word");
                __builtin_amdgcn_raw_buffer_store_b32(((field[1] << 16) | (field[0] & 0xFFFFu)) ^ 0x88888888u, yr, ovoff, 0, 0);
            }
            ovoff += orowb;
        };
#define STRIP_BODY(J) body(X[(J) % 3], X[((J) + 1) % 3], X[((J) + 2) % 3], raw[(J) % D], rs[(J) % D], rf[(J) % D])
        int yy = y0;
        for (; yy + D <= y1; yy += D) {
            STRIP_BODY(0); STRIP_BODY(1); STRIP_BODY(2);
            if constexpr (D > 3) { STRIP_BODY(3); STRIP_BODY(4); STRIP_BODY(5); }
            if constexpr (D > 6) { STRIP_BODY(6); STRIP_BODY(7); STRIP_BODY(8); }
            if constexpr (D > 9) { STRIP_BODY(9); STRIP_BODY(10); STRIP_BODY(11); }
        }
        static_assert(D <= 12, "unrolled by hand up to twelve rows");
        const int rem = y1 - yy;
        if (rem > 0) STRIP_BODY(0);
        if (rem > 1) STRIP_BODY(1);
        if constexpr (D > 3) { if (rem > 2) STRIP_BODY(2); if (rem > 3) STRIP_BODY(3); if (rem > 4) STRIP_BODY(4); }
        if constexpr (D > 6) { if (rem > 5) STRIP_BODY(5); if (rem > 6) STRIP_BODY(6); if (rem > 7) STRIP_BODY(7); }
        if constexpr (D > 9) { if (rem > 8) STRIP_BODY(8); if (rem > 9) STRIP_BODY(9); if (rem > 10) STRIP_BODY(10); }
#undef STRIP_BODY
    }
}

// ---------------------------------------------------------------------------------------------------------
// The stride-2 3x3 layers that open a ResNet stage (models/resnet.py:108-112; no residual merge behind them): the same
// strip walk over OUTPUT rows; an output row needs input rows 2*yy - pt .. + 2, of which only one is shared with the next
// output row, so every output row simply requests its three input rows (one output row ahead) and widens them.
// B operand of lane (pixel r, k-block): input pixel 2*(xs + r) - pl + dx.
// ---------------------------------------------------------------------------------------------------------
template <int CIN, int NT, bool BIAS, int FOLD, int FN = 0>
__global__ __launch_bounds__(256, (CIN == 16 ? 4 : 2)) void k_conv_strip_s2(MfmaGeom mg, EpiArgs e,
                                                                             const uint8_t* __restrict__ x,
                                                                             const uint8_t* __restrict__ wq8,
                                                                             void* __restrict__ y, int ntasks, int spr,
                                                                             FastDiv fd_spr, int nch, FastDiv fd_nch,
                                                                             int rc, uint32_t img_x, uint32_t img_y) {
    constexpr int BP = CIN / 16;
    constexpr int ST = BP;                             // tap dx = kq, channel group st (see k_conv_strip)
    constexpr int PIXB = CIN / 2;
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
    v4i bw[3][ST][NT];                                 // as in k_conv_strip: consecutive channels per lane
    strip_load_filters<CIN>(bw, wq8, mg.w_bytes, nbase, r, kok, dxs, hbs);
    static_assert(NT == 2, "the stride-2 kernel stores one 32-bit word per lane");
    static_assert(!FOLD || FN == 0, "only quantized_tanh is folded");
    const bool binary = e.fn == QNN_FN_BINARY_TANH;
    const float cfold = binary ? 1.0f : e.act_m;
    v2f nb[NT][2], ninv[NT][2], nshift[NT][2];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = nbase + 4 * NT * kq + 4 * nt + i;
            nb[nt][i >> 1][i & 1] = BIAS ? __fdiv_rn(e.bias[c], e.scale) : 0.0f;
            ninv[nt][i >> 1][i & 1] = __fmul_rn(__fmul_rn(e.bn_inv ? e.bn_inv[c] : 1.0f, e.scale), cfold);
            nshift[nt][i >> 1][i & 1] = __fmul_rn(e.bn_inv ? e.bn_shift[c] : 0.0f, cfold);
        }
    float fa[NT][4], fc[NT][4];                        // folded epilogue (k_conv_strip): slope, constant and accumulator offset
    v4i binit[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = nbase + 4 * NT * kq + 4 * nt + i;
            fa[nt][i] = FOLD ? e.fold_a[c] : 0.0f;
            fc[nt][i] = FOLD == 2 ? e.fold_c[c] : 0.0f;
            binit[nt][i] = FOLD ? e.fold_b[c] : 0;
        }
    constexpr float kMagic = 12582920.0f;
    constexpr int kMagicBits = 0x4B400008;
    const float mgc = FN == QNN_FN_QUANTIZED_RELU ? kMagic - e.act_m : kMagic;     // (an even integer either way: act_bits >= 2)
    v2f magic2 = {mgc, mgc};
    asm volatile("" : "+v"(magic2));                  // a register pair (v_pk_add_f32 takes no literal): keeps the add packed
    const int code_lo = FN == QNN_FN_QUANTIZED_RELU ? kMagicBits : kMagicBits - (int)e.act_m, code_hi = kMagicBits + (int)e.act_m - 1;
    const v2f act_m2 = {e.act_m, e.act_m}, alpha2 = {0.1f, 0.1f};      // strip_qact<FN>; unused for FN = 0
    const int rowb2 = 2 * g.W * PIXB;                  // two input rows per output row
    const int orowb = g.Wo * e.ocw * 4;
    for (int task = wid; task < ntasks; task += nw) {
        const StripTask tk = strip_task(task, fd_nch, nch, fd_spr, spr, rc, g.Ho);
        const int n = tk.n, xs = tk.xs, y0 = tk.y0, y1 = tk.y1;
        const __amdgpu_buffer_rsrc_t xr = strip_image_rsrc(x, n, img_x), yr = strip_image_rsrc(y, n, img_y);
        int voff[3];
        const int px = 2 * (xs + r) - g.pl + kq;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
            voff[dy] = (kq < 3 && px >= 0 && px < g.W && xs + r < g.Wo) ? ((2 * y0 - g.pt + dy) * g.W + px) * PIXB
                                                                        : (int)0x80000000;
        const bool pvalid = xs + r < g.Wo;
        int ovoff = pvalid ? (y0 * g.Wo + xs + r) * e.ocw * 4 + nbase / 2 + kq * 2 * NT : (int)0x80000000;
        uint2 raw[2][3][ST];
        auto load_rows = [&](uint2 (&dst)[3][ST]) {
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
                if constexpr (BP == 1) {
                    dst[dy][0] = __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(xr, voff[dy], 0, 0));
                } else {
#pragma unroll
                    for (int h = 0; h < BP / 2; ++h) {
                        const uint4 v = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(xr, voff[dy] + 16 * h, 0, 0));
                        dst[dy][2 * h] = make_uint2(v.x, v.y);
                        dst[dy][2 * h + 1] = make_uint2(v.z, v.w);
                    }
                }
                voff[dy] += rowb2;
            }
        };
        load_rows(raw[0]);
        auto body = [&](uint2 (&cur)[3][ST], uint2 (&nxt)[3][ST]) {
            load_rows(nxt);                            // the three input rows of the next output row
            v4i acc[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[nt] = binit[nt];
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int st = 0; st < ST; ++st) {
                    const v4i xo = strip_widen(cur[dy][st]);
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
                        acc[nt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(bw[dy][st][nt], xo, acc[nt], 0, 0, 0);
                }
            if constexpr (FOLD) {
                uint32_t tp[4];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    tp[j] = qnn_fold_pair_m<FOLD>(acc[0][j], acc[1][j], fa[0][j], fa[1][j], fc[0][j], fc[1][j]);   // (c_j, c_j+4)
                const uint32_t uo = __builtin_amdgcn_perm(tp[3], tp[1], 0x07030501u);
                const uint32_t ue = __builtin_amdgcn_perm(tp[2], tp[0], 0x07030501u);
                __builtin_amdgcn_raw_buffer_store_b32((uo & 0xF0F0F0F0u) | ((ue >> 4) & 0x0F0F0F0Fu), yr, ovoff, 0, 0);
                ovoff += orowb;
                return;
            }
            uint32_t field[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                v2f u2[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    v2f v = {(float)acc[nt][2 * h], (float)acc[nt][2 * h + 1]};
                    if constexpr (BIAS) v = v + nb[nt][h];
                    u2[h] = v * ninv[nt][h];
                    u2[h] = u2[h] + nshift[nt][h];
                }
                int cb[4];
                strip_qact<FN>(u2, act_m2, alpha2);
                if (FN == 0 && binary) {
                    asm volatile("; binary_tanh codes");
#pragma unroll
                    for (int i = 0; i < 4; ++i) cb[i] = u2[i >> 1][i & 1] > 0x1p-24f ? kMagicBits + 1 : kMagicBits - 1;
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
                uint32_t P = ((uint32_t)cb[1] << 4) | (uint32_t)cb[0];
                P = ((uint32_t)cb[2] << 8) | P;
                P = ((uint32_t)cb[3] << 12) | P;
                field[nt] = P;
            }
            __builtin_amdgcn_raw_buffer_store_b32(((field[1] << 16) | (field[0] & 0xFFFFu)) ^ 0x88888888u, yr, ovoff, 0, 0);
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

// FN of the kernels for this call's activation (0: quantized_tanh / binary_tanh)
inline int strip_fn(const EpiArgs& e) {
    return e.fn == QNN_FN_QUANTIZED_RELU || e.fn == QNN_FN_QUANTIZED_LEAKYRELU ? e.fn : 0;
}

template <int CIN, int NT>
int launch_strip_s2(const MfmaGeom& mg, const EpiArgs& e, const void* x, const uint8_t* w, void* y, hipStream_t s) {
    const ConvGeom& g = mg.g;
    const int spr = (g.Wo + 15) / 16;
    const int ny = g.cout / (16 * NT);
    const double img_x = (double)g.H * g.W * (CIN / 2), img_y = (double)g.Ho * g.Wo * e.ocw * 4.0;
    if (img_x >= 1.0e9 || img_y >= 1.0e9 || ny < 1 || ny * 16 * NT != g.cout) return 1;
    const int wps = CIN == 16 ? 4 : 2;
    StripPlan p;                // over output rows
    if (!qnn_strip_plan(&p, g.N, spr, g.Ho, 256 * wps / ny > 0 ? 256 * wps / ny : 1, 2, 1)) return 1;
    const dim3 grid(p.blocks, (unsigned)ny), block(256);
    // a fold contains the bias: "bits" form (2), float form (1), else the plain epilogue with or without a bias
    const int fold = !e.fold_a ? 0 : e.fold_c ? 2 : 1;
    const bool bias = !fold && e.bias;
    const int qfn = strip_fn(e);
    if (fold && qfn) return 1;  // (not reached: no fold is prepared for these activations)
#define STRIP_S2_CASE(BIAS_, FOLD_, FN_)                                                                                  \
    if (bias == BIAS_ && fold == FOLD_ && qfn == FN_) {                                                                   \
        hipLaunchKernelGGL((k_conv_strip_s2<CIN, NT, BIAS_, FOLD_, FN_>), grid, block, 0, s, mg, e, (const uint8_t*)x, w, y, \
                           QNN_STRIP_PLAN_ARGS(p), (uint32_t)img_x, (uint32_t)img_y);                                     \
        return 0;                                                                                                         \
    }
    STRIP_S2_CASE(false, 2, 0) STRIP_S2_CASE(false, 1, 0) STRIP_S2_CASE(true, 0, 0) STRIP_S2_CASE(false, 0, 0)
    STRIP_S2_CASE(true, 0, QNN_FN_QUANTIZED_RELU) STRIP_S2_CASE(false, 0, QNN_FN_QUANTIZED_RELU)
    STRIP_S2_CASE(true, 0, QNN_FN_QUANTIZED_LEAKYRELU) STRIP_S2_CASE(false, 0, QNN_FN_QUANTIZED_LEAKYRELU)
#undef STRIP_S2_CASE
    return 1;                   // not reached: (bias, fold) takes exactly the four values above
}

template <int CIN, int NT>
int launch_strip(const MfmaGeom& mg, const EpiArgs& e, const void* x, const uint8_t* w, void* y, hipStream_t s) {
    const ConvGeom& g = mg.g;
    const int spr = (g.W + 15) / 16;
    const int ny = g.cout / (16 * NT);
    const double img_x = (double)g.H * g.W * (CIN / 2), img_y = (double)g.H * g.W * e.ocw * 4.0;
    const int res = e.proj_x ? 3 : !e.res ? 0 : e.res_store == QNN_STORE_F32 ? 2 : 1;
    const double img_r = res == 2 ? (double)g.H * g.W * g.cout * 4.0
                         : res == 3 ? (double)e.proj_H * e.proj_W * (CIN / 4) : img_y;
    if (res == 3 && (NT != 2 || CIN < 32 || e.proj_cin * 2 != CIN)) return 1;
    if (img_x >= 1.0e9 || img_y >= 1.0e9 || img_r >= 1.0e9 || ny < 1 || ny * 16 * NT != g.cout) return 1;
    // persistent grid: WPS waves per SIMD.  Both arguments are known to be stale and kept as measured (changing them
    // changes grid sizes): the fill of 3 rows dates from the three-row ring, today's ring of D rows fills in D + 2; and
    // the float32-residual (RES 2) kernels of the 32-channel stage are bounded for two waves per SIMD while wps says 1.
    const int wps = CIN == 16 ? QNN_STRIP16_WPS : CIN == 32 ? QNN_STRIP32_WPS : QNN_STRIP64_WPS;
    StripPlan p;
    if (!qnn_strip_plan(&p, g.N, spr, g.H, 256 * wps / ny > 0 ? 256 * wps / ny : 1, 3, 1)) return 1;
    const dim3 grid(p.blocks, (unsigned)ny), block(256);
    const bool bias = e.bias != nullptr && !(e.fold_a != nullptr && res < 2);   // a fold contains the bias
#define STRIP_CASE_FN(RES_, BIAS_, FOLD_, FN_)                                                                \
    if (res == RES_ && bias == BIAS_ && fold == FOLD_ && qfn == FN_) {                                        \
        hipLaunchKernelGGL((k_conv_strip<CIN, NT, RES_, BIAS_, FOLD_, FN_>), grid, block, 0, s, mg, e, (const uint8_t*)x, w, y, \
                           QNN_STRIP_PLAN_ARGS(p), (uint32_t)img_x, (uint32_t)img_y, (uint32_t)img_r);       \
        return 0;                                                                                             \
    }
#define STRIP_CASE(RES_, BIAS_, FOLD_) STRIP_CASE_FN(RES_, BIAS_, FOLD_, 0)
    // the un-folded chain with each activation (a fold exists for quantized_tanh only)
#define STRIP_CASE3(RES_, BIAS_)                                                                              \
    STRIP_CASE_FN(RES_, BIAS_, 0, 0) STRIP_CASE_FN(RES_, BIAS_, 0, QNN_FN_QUANTIZED_RELU)                     \
    STRIP_CASE_FN(RES_, BIAS_, 0, QNN_FN_QUANTIZED_LEAKYRELU)
    const int qfn = strip_fn(e);
    // folded epilogue: everything behind the accumulator (bias included) is inside the fold's two constants
    const int fold = (e.fold_a == nullptr || res >= 2) ? 0 : e.fold_c ? 2 : 1;
    STRIP_CASE(0, false, 2) STRIP_CASE(1, false, 2) STRIP_CASE(0, false, 1) STRIP_CASE(1, false, 1)
    if (fold && qfn) return 1;  // (not reached: no fold is prepared for these activations)
    STRIP_CASE3(0, false) STRIP_CASE3(0, true) STRIP_CASE3(1, false) STRIP_CASE3(1, true)
    STRIP_CASE3(2, false) STRIP_CASE3(2, true)
    if constexpr (NT == 2 && CIN >= 32) { STRIP_CASE3(3, false) STRIP_CASE3(3, true) }
#undef STRIP_CASE3
#undef STRIP_CASE
#undef STRIP_CASE_FN
    return 1;
}

}  // namespace

// cin in {16, 32, 64}, cout a multiple of 16 / 32 / 32; eligibility is checked by the caller
int qnn_launch_strip(int cin, const MfmaGeom& mg, const EpiArgs& e, const void* x, const uint8_t* w,
                     void* y, hipStream_t s) {
    if (mg.g.stride == 2) {
        if (e.res) return 1;
        return cin == 16 ? launch_strip_s2<16, 2>(mg, e, x, w, y, s) : cin == 32 ? launch_strip_s2<32, 2>(mg, e, x, w, y, s) : 1;
    }
    if (cin == 16) return launch_strip<16, 1>(mg, e, x, w, y, s);
    if (cin == 32) return launch_strip<32, 2>(mg, e, x, w, y, s);
    return launch_strip<64, 2>(mg, e, x, w, y, s);
}
