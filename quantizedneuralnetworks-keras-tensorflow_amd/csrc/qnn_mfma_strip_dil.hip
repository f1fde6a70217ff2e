// 3x3 stride-1 'same' int4 layers with 16 / 32 / 64 input channels and a DILATED window (dilation_rate d x d of the
// reference's conv layers, quantized_layers.py:171-177): the dilated counterpart of k_conv_strip (qnn_mfma_strip.hip) on
// v_mfma_i32_16x16x64_i8.  Dispatch: qnn_route_strip_dil, at the end of this file; every other dilated call runs on
// k_conv_generic, and this kernel is bit-identical to it (exact integer sums, then the float32 chain in the reference's
// op order, as the unfolded k_conv_strip evaluates it).
//
// What is kept from k_conv_strip: A = filters, B = pixels; a wave walks a 16-pixel column strip of ONE image down a
// chunk of rows (tasks from qnn_strip_plan); a lane holds 4 * NT consecutive channels of one pixel and stores them with
// one 2- or 4-byte store; the same K order (block j = (tap dx = j / BP, channel group j % BP), K-step st takes
// j = 4 * st + kq); every tensor is addressed through a buffer descriptor of one image, so rows above the first and
// below the last read as zeros and a tap never reaches the neighbouring image.
//
// What dilation changes:
//   * An input row r serves the output rows r - d, r, r + d.  The widened operands of R = 2d + 1 input rows live in a
//     register ring; output row yy multiplies slots of rows yy - d / yy / yy + d with filter rows 0 / 1 / 2, and the
//     row yy + d widened here replaces row yy - d - 1.  The row loop is unrolled R times, so that every slot is a
//     compile-time register name.
//   * The horizontal taps sit at columns c - d, c, c + d.  A lane's k-block of K-step st belongs to ONE tap dx, so its
//     column c + (dx - 1) d is fixed for the whole strip: the lane gets an out-of-range offset for that K-step once per
//     strip where the column is outside the image.  Up to d lanes at either end of a row are such lanes, and in an
//     image narrower than d every side tap of every lane is.  Nothing is masked inside the loop.
//   * Raw rows are requested R rows ahead of the row being widened (the ring of k_conv_strip, depth R).
// No fold and no in-launch projection: qnn_prepack_weights_dilated / check_epilogue refuse both for a dilated handle.
#include <math.h>
#include <stdio.h>

#include <type_traits>

#include "qnn_mfma_common.h"
#include "qnn_strip_plan.h"
#include "qnn_strip_device.h"

namespace {

// waves per SIMD (= persistent workgroups per CU) the kernels are bounded for; VGPR counts in DESIGN 3.2
constexpr int dil_wps(int cin) { return cin == 16 ? 4 : cin == 32 ? 2 : 1; }

template <int J, int N, typename F>
__device__ __forceinline__ void dil_static_for(F&& f) {
    if constexpr (J < N) {
        f(std::integral_constant<int, J>{});
        dil_static_for<J + 1, N>(f);
    }
}

// RES: 0 none, 1 packed int4 shortcut, 2 float32 shortcut (post_scale a power of two: it folds into the code scale)
template <int CIN, int NT, int DIL, int RES, bool BIAS>
__global__ __launch_bounds__(256, dil_wps(CIN)) void k_conv_strip_dil(MfmaGeom mg, EpiArgs e, const uint8_t* __restrict__ x,
                                                                      const uint8_t* __restrict__ wq8, void* __restrict__ y,
                                                                      int ntasks, int spr, FastDiv fd_spr, int nch,
                                                                      FastDiv fd_nch, int rc, uint32_t img_x, uint32_t img_y,
                                                                      uint32_t img_r) {
    constexpr int BP = CIN / 16;                      // 16-channel k-blocks per pixel
    constexpr int ST = (3 * BP + 3) / 4;              // K-steps per input row: 1 / 2 / 3
    constexpr int PIXB = CIN / 2;                     // bytes per stored input pixel
    constexpr int R = 2 * DIL + 1;                    // input rows alive at once
    static_assert(NT <= 2, "a lane's fields must fit one word");
    const ConvGeom& g = mg.g;
    const int lane = threadIdx.x & 63;
    const int r = lane & 15, kq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int wid = blockIdx.x * 4 + wave, nw = gridDim.x * 4;
    const int nbase = blockIdx.y * (16 * NT);         // first output channel of this wave

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
    // ---- filters: A operand, row = output channel; a lane's 4 * NT results are consecutive channels (k_conv_strip) ----
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
    // ---- epilogue constants of this lane's channels nbase + 4*NT*kq + 4*nt + i: the powers of two behind the BN
    // (activation code scale, residual post-scale) commute with every rounding and are folded in, as in k_conv_strip ----
    const bool binary = e.fn == QNN_FN_BINARY_TANH;
    const float cfold = (RES != 0 ? e.post_scale : 1.0f) * (binary ? 1.0f : e.act_m);
    const float rcoef = RES == 1 ? e.res_scale * cfold : cfold;
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
    // round-half-even + clamp + offset code in the integer domain (k_conv_strip): the low nibble is code + 8
    constexpr float kMagic = 12582920.0f;
    constexpr int kMagicBits = 0x4B400008;
    v2f magic2 = {kMagic, kMagic};
    asm volatile("" : "+v"(magic2));                  // a register pair (v_pk_add_f32 takes no literal): keeps the add packed
    const int code_lo = kMagicBits - (int)e.act_m, code_hi = kMagicBits + (int)e.act_m - 1;
    const int rowb = g.W * PIXB;                      // bytes per input row
    const int orowb = g.W * e.ocw * 4;                // bytes per output row
    const int rrowb = RES == 2 ? g.W * g.cout * 4 : orowb;

    for (int task = wid; task < ntasks; task += nw) {
        const StripTask tk = strip_task(task, fd_nch, nch, fd_spr, spr, rc, g.H);
        const int n = tk.n, xs = tk.xs, y0 = tk.y0, y1 = tk.y1;
        const __amdgpu_buffer_rsrc_t xr = strip_image_rsrc(x, n, img_x), yr = strip_image_rsrc(y, n, img_y);
        const __amdgpu_buffer_rsrc_t rr = RES == 0 ? strip_image_rsrc(y, 0, 0) : strip_image_rsrc(e.res, n, img_r);
        // byte offset (inside the image) of this lane's k-block in input row y0 - d: negative above the image (out of
        // range as an unsigned offset, in range again from row 0 on); a tap column left or right of the image starts
        // out of range and stays there (0x80000000 + row increments < 2^32, images are < 10^9 bytes)
        int voff[ST];
#pragma unroll
        for (int st = 0; st < ST; ++st) {
            const int px = xs + r + (dxs[st] - 1) * DIL;
            voff[st] = (kok[st] && px >= 0 && px < g.W) ? ((y0 - DIL) * g.W + px) * PIXB + hbs[st] * 8 : (int)0x80000000;
        }
        const bool pvalid = xs + r < g.W;                                       // last strip of a ragged row
        int ovoff = pvalid ? (y0 * g.W + xs + r) * e.ocw * 4 + nbase / 2 + kq * 2 * NT : (int)0x80000000;   // 2*NT bytes
        int rvoff = RES == 2 ? (pvalid ? ((y0 * g.W + xs + r) * g.cout + nbase + 4 * NT * kq) * 4 : (int)0x80000000) : ovoff;

        v4i X[R][ST];                                  // slot (row - (y0 - d)) mod R
        uint2 raw[R][ST];                              // rows requested ahead: slot j mod R holds row y0 + d + j
        auto load_row = [&](uint2 (&dst)[ST]) {
#pragma unroll
            for (int st = 0; st < ST; ++st) {
                dst[st] = __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(xr, voff[st], 0, 0));
                voff[st] += rowb;
            }
        };
        {
            uint2 t[2 * DIL][ST];
#pragma unroll
            for (int i = 0; i < 2 * DIL; ++i) load_row(t[i]);                   // rows y0 - d .. y0 + d - 1
#pragma unroll
            for (int i = 0; i < R; ++i) load_row(raw[i]);                       // rows y0 + d .. y0 + 3d
#pragma unroll
            for (int i = 0; i < 2 * DIL; ++i)
#pragma unroll
                for (int st = 0; st < ST; ++st) X[i][st] = strip_widen(t[i][st]);
        }

        // one output row yy = y0 + j: X slots j, j + d, j + 2d (mod R) hold input rows yy - d / yy / yy + d; ring slot
        // j mod R holds row yy + d (widened here, refilled with row yy + d + R)
        auto body = [&](v4i (&Xa)[ST], v4i (&Xb)[ST], v4i (&Xc)[ST], uint2 (&rw)[ST]) {
            uint32_t rcur = 0;
            float4 fcur[NT];
            if constexpr (RES == 1) {                  // the lane's whole 2*NT-byte field of shortcut codes
                if constexpr (NT == 1) rcur = __builtin_amdgcn_raw_buffer_load_b16(rr, rvoff, 0, 0);
                else rcur = __builtin_amdgcn_raw_buffer_load_b32(rr, rvoff, 0, 0);
            }
            if constexpr (RES == 2) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    fcur[nt] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rr, rvoff + 16 * nt, 0, 0));
            }
            if constexpr (RES != 0) rvoff += rrowb;
#pragma unroll
            for (int st = 0; st < ST; ++st) Xc[st] = strip_widen(rw[st]);
            load_row(rw);                              // row yy + d + R
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
            // ---- epilogue: the reference's op order, one rounding per operation (the unfolded chain of k_conv_strip) ----
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
                        const v2f cd = {(float)((int)(rcur << (28 - 8 * h - 16 * nt)) >> 28),
                                        (float)((int)(rcur << (24 - 8 * h - 16 * nt)) >> 28)};
                        u = __builtin_elementwise_fma(cd, rcoef2, u);
                    }
                    if constexpr (RES == 2) {
                        const v2f rv = h == 0 ? v2f{fcur[nt].x, fcur[nt].y} : v2f{fcur[nt].z, fcur[nt].w};
                        u = __builtin_elementwise_fma(rv, rcoef2, u);   // (x + y) * 2^k == x*2^k + y*2^k, one rounding either way
                    }
                    u2[h] = u;
                }
                int cb[4];
                if (binary) {
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
                __builtin_amdgcn_raw_buffer_store_b32(((field[NT - 1] << 16) | (field[0] & 0xFFFFu)) ^ 0x88888888u, yr, ovoff, 0, 0);
            }
            ovoff += orowb;
        };
        for (int yy = y0; yy < y1; yy += R)
            dil_static_for<0, R>([&](auto jc) {
                constexpr int J = decltype(jc)::value;
                if (yy + J < y1) body(X[J % R], X[(J + DIL) % R], X[(J + 2 * DIL) % R], raw[J % R]);
            });
    }
}

template <int CIN, int NT, int DIL>
int launch_strip_dil(const MfmaGeom& mg, const EpiArgs& e, const void* x, const uint8_t* w, void* y, hipStream_t s) {
    const ConvGeom& g = mg.g;
    const int spr = (g.W + 15) / 16;
    const int ny = g.cout / (16 * NT);
    const double img_x = (double)g.H * g.W * (CIN / 2), img_y = (double)g.H * g.W * e.ocw * 4.0;
    const int res = !e.res ? 0 : e.res_store == QNN_STORE_F32 ? 2 : 1;
    const double img_r = res == 2 ? (double)g.H * g.W * g.cout * 4.0 : img_y;
    if (img_x >= 1.0e9 || img_y >= 1.0e9 || img_r >= 1.0e9 || ny < 1 || ny * 16 * NT != g.cout) return 1;
    // persistent grid of dil_wps waves per SIMD; a task fills its ring in 2d + 2 rows before the first store
    const int cap = 256 * dil_wps(CIN) / ny;
    StripPlan p;
    if (!qnn_strip_plan(&p, g.N, spr, g.H, cap > 0 ? cap : 1, 2 * DIL + 2, 1)) return 1;
    const dim3 grid(p.blocks, (unsigned)ny), block(256);
    const bool bias = e.bias != nullptr;
#define STRIP_DIL_CASE(RES_, BIAS_)                                                                                   \
    if (res == RES_ && bias == BIAS_) {                                                                               \
        hipLaunchKernelGGL((k_conv_strip_dil<CIN, NT, DIL, RES_, BIAS_>), grid, block, 0, s, mg, e, (const uint8_t*)x, w, y, \
                           QNN_STRIP_PLAN_ARGS(p), (uint32_t)img_x, (uint32_t)img_y, (uint32_t)img_r);               \
        return 0;                                                                                                     \
    }
    STRIP_DIL_CASE(0, false) STRIP_DIL_CASE(0, true) STRIP_DIL_CASE(1, false) STRIP_DIL_CASE(1, true)
    STRIP_DIL_CASE(2, false) STRIP_DIL_CASE(2, true)
#undef STRIP_DIL_CASE
    return 1;                   // not reached: (res, bias) takes exactly the six values above
}

template <int DIL>
int launch_strip_dil_cin(int cin, const MfmaGeom& mg, const EpiArgs& e, const void* x, const uint8_t* w, void* y,
                         hipStream_t s) {
    if (cin == 16) return launch_strip_dil<16, 1, DIL>(mg, e, x, w, y, s);
    if (cin == 32) return launch_strip_dil<32, 2, DIL>(mg, e, x, w, y, s);
    return launch_strip_dil<64, 2, DIL>(mg, e, x, w, y, s);
}

}  // namespace

// The dilated calls this file runs; every other one falls to k_conv_generic.  Shape: 3x3, stride 1, 'same' (pt = pl = d),
// SQUARE dilation d in {2, 3} -- the two instantiations of the kernel --, int4 codes in and out, un-pooled, Cin 16 / 32 /
// 64, Cout a multiple of 16 (Cin 16) or 32; an optional residual as packed int4 codes of the output's layout or float32,
// with a power-of-two post_scale.  No fold, no projection (refused for a dilated handle before any route is asked), no
// identity trick (CAP_TRICK is not among this route's capabilities).
int qnn_route_strip_dil(const ConvCall& c, char* name, size_t name_len) {
    const ConvGeom& g = c.g;
    const EpiArgs& e = c.e;
    const qnn_weights* w = c.w;
    if (!w->d_mfma || c.x_store != QNN_STORE_I4 || w->store != QNN_STORE_I4 || (e.flags & QNN_EPI_NO_STRIP)) return 1;
    const int d = g.dil_h;
    int pexp = 0;
    const bool pow2 = !e.res || (e.post_scale > 0.0f && frexpf(e.post_scale, &pexp) == 0.5f);
    const bool shape = (d == 2 || d == 3) && g.dil_w == d && g.kh == 3 && g.kw == 3 && g.stride == 1 && g.pt == d &&
                       g.pl == d && g.Ho == g.H && g.Wo == g.W && g.pool == 1 &&
                       (g.cin == 16 || g.cin == 32 || g.cin == 64) && (g.cout % (g.cin == 16 ? 16 : 32)) == 0 &&
                       e.out_store == QNN_STORE_I4 && pow2 &&
                       (e.fn == QNN_FN_QUANTIZED_TANH || e.fn == QNN_FN_BINARY_TANH) &&
                       (!e.res || (e.res_store == QNN_STORE_I4 && e.res_cw == e.ocw) ||
                        (e.res_store == QNN_STORE_F32 && e.res_cw == g.cout));
    const double wb = (double)g.cout * 9 * g.cin;
    if (!shape || wb >= 2.0e9) return 1;
    MfmaGeom ms;
    ms.g = g; ms.kc = 1; ms.steps = 0; ms.x_pix_bytes = g.cin / 2; ms.total_q = (long)g.N * g.H * g.W;
    ms.x_bytes = 0; ms.w_bytes = (uint32_t)wb;
    EpiArgs es = e;
    es.scale = e.scale * (1.0f / 256.0f);                    // both operands carry *16
    snprintf(name, name_len, "strip_i4_c%d_dil", g.cin);
    return d == 2 ? launch_strip_dil_cin<2>(g.cin, ms, es, c.x, w->d_mfma, c.y, c.s)
                  : launch_strip_dil_cin<3>(g.cin, ms, es, c.x, w->d_mfma, c.y, c.s);
}
