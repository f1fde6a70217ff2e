// Route of the row-walking strip family: 3x3 layers with 16 / 32 / 64 input channels and an un-pooled packed output of
// the input's own width (int4 -> int4: qnn_mfma_strip.hip, qnn_mfma_strip16.hip; int8 -> int8: qnn_mfma_strip_i8.hip),
// then the small-channel tile kernel (qnn_mfma_small.hip).  Host code only: this file holds no kernel.
// quantized_relu / quantized_leakyrelu (the route's CAP_QACT): the un-folded int4 strip kernels of qnn_mfma_strip.hip
// implement them; the int8 strips, the LDS-staged 16-channel form and the tile kernel decline such a call.
#include <math.h>
#include <stdio.h>

#include "qnn_mfma_common.h"

// The layer shapes the strip kernels of either width run; `store` = QNN_STORE_I4 or QNN_STORE_I8, of input, output and a
// packed residual alike.
static bool strip_qact(const EpiArgs& e) {
    return e.fn == QNN_FN_QUANTIZED_RELU || e.fn == QNN_FN_QUANTIZED_LEAKYRELU;
}

static bool strip_shape(const ConvGeom& g, const EpiArgs& e, int store) {
    int pexp = 0;
    // the residual's post-scale (models/resnet.py:128: 0.5) folds into the activation's code scale: a power of two
    const bool pow2 = (!e.res && !e.proj_x) || (e.post_scale > 0.0f && frexpf(e.post_scale, &pexp) == 0.5f);
    const int cmul = g.cin == 16 ? 16 : 32;
    const bool s1 = g.stride == 1 && g.pt == 1 && g.pl == 1 && (g.cout % cmul) == 0;
    // stride 2 (the first conv of a stage: no residual, Cin 16 / 32, Cout a multiple of 32): the same walk over output
    // rows, three fresh input rows per output row
    const bool s2 = g.stride == 2 && (g.cin == 16 || g.cin == 32) && (g.cout % 32) == 0 && !e.res;
    return (g.cin == 16 || g.cin == 32 || g.cin == 64) && g.kh == 3 && g.kw == 3 && (s1 || s2) && g.pool == 1 &&
           e.out_store == store && pow2 &&
           (!e.res || (e.res_store == store && e.res_cw == e.ocw) || (e.res_store == QNN_STORE_F32 && e.res_cw == g.cout));
}

// Geometry of a launch that needs no K loop (one 3x3 window per output pixel); false: past the 31-bit buffer offsets.
// Only the tile kernel reads x through a sized descriptor (with_x_bytes).
static bool strip_geom(MfmaGeom* ms, const ConvGeom& g, int x_pix_bytes, long total_q, bool with_x_bytes) {
    ms->g = g; ms->kc = 1; ms->steps = 0; ms->x_pix_bytes = x_pix_bytes;
    ms->total_q = total_q;
    const double xb = with_x_bytes ? (double)g.N * g.H * g.W * x_pix_bytes : 0.0, wb = (double)g.cout * 9 * g.cin;
    if (xb >= 2.0e9 || wb >= 2.0e9) return false;
    ms->x_bytes = (uint32_t)xb; ms->w_bytes = (uint32_t)wb;
    return true;
}

// int8-stored activations and weights, un-pooled int8 output: the int8 strip kernels.  Everything else with int8
// operands stays where it was: pooled layers and Cin = 64 on the tiled family (qnn_route_gemm), float32 or int4 outputs
// and 16 / 32 channels on k_conv_ps.
static int route_strip_i8(const ConvCall& c, char* name, size_t name_len) {
    const ConvGeom& g = c.g;
    const EpiArgs& e = c.e;
    // no folded epilogue and no in-launch projection in the int8 kernels
    if (c.w->store != QNN_STORE_I8 || (e.flags & QNN_EPI_NO_STRIP) || e.fold_a || e.proj_x || strip_qact(e)) return 1;
    // Accumulator bound: K = 9 * Cin <= 576 products of two codes in [-128, 127]: |acc| <= 576 * 128 * 128 = 9 437 184
    // < 2^24, so the kernels' int -> float32 conversion is exact (as the reference's float32 sum of the same products).
    static_assert(576L * 128 * 128 < (1L << 24), "int8 strip kernels: accumulators must convert to float32 exactly");
    // Cin 64 has a matrix-pipe kernel already (mfma_i8_areg64x64 for Cout = 64): QNN_EPI_NO_STRIP64 keeps it, as on the
    // int4 path; the two times are in DESIGN 3.2
    const bool want = g.cin != 64 || !(e.flags & QNN_EPI_NO_STRIP64);
    MfmaGeom ms;
    if (!strip_shape(g, e, QNN_STORE_I8) || !want || !strip_geom(&ms, g, g.cin, (long)g.N * g.Ho * g.Wo, false)) return 1;
    snprintf(name, name_len, g.stride == 2 ? "strip_i8_c%d_s2" : "strip_i8_c%d", g.cin);
    return qnn_launch_strip_i8(g.cin, ms, e, c.x, c.w->d_mfma, c.y, c.s);
}

int qnn_route_strip(const ConvCall& c, char* name, size_t name_len) {
    const ConvGeom& g = c.g;
    const EpiArgs& e = c.e;
    const qnn_weights* w = c.w;
    if (!w->d_mfma) return 1;
    if (c.x_store == QNN_STORE_I8) return route_strip_i8(c, name, name_len);
    if (c.x_store != QNN_STORE_I4 || w->store != QNN_STORE_I4) return 1;
    MfmaGeom ms;
    EpiArgs es = e;
    es.scale = e.scale * (1.0f / 256.0f);                    // both operands carry *16
    // the in-launch projection shortcut: stride 1, 32 / 64 channels, the block input at twice the size and half the
    // channels, instead of a residual and without a fold
    const bool proj_ok = !e.proj_x || (g.stride == 1 && (g.cin == 32 || g.cin == 64) && g.cout == g.cin && e.proj_cin * 2 == g.cin &&
                                       !e.res && !e.fold_a && (e.proj_H + 1) / 2 == g.H && (e.proj_W + 1) / 2 == g.W);
    const bool qact = strip_qact(e);                         // never with a fold (check_epilogue)
    // Cin 64 (auto): every un-pooled layer.  Measured, 64 x 56^2 / 4096 x 16^2 pixels, round 3 (one 32-bit store and one
    // shortcut load per row): with the merge 13.9 us here against 36.4 us on the LDS-weight kernel, without it
    // 13.1 / 43.5 against 14.0 / 46.5 (round 2, two 16-bit accesses per row: 16.3 / 54.6 against 14.1 / 47.3).
    const bool want = g.cin != 64 || !(e.flags & QNN_EPI_NO_STRIP64);
    if (strip_shape(g, e, QNN_STORE_I4) && proj_ok && want && !(e.flags & QNN_EPI_NO_STRIP) &&
        strip_geom(&ms, g, g.cin / 2, (long)g.N * g.H * g.W, false)) {
        EpiArgs ep = es;
        ep.proj_scale = e.proj_scale * (1.0f / 256.0f);      // the projection's operands too
        // 16 -> 16 channels with a usable fold and an even width: the LDS-staged form (qnn_mfma_strip16.hip: a sixth
        // of the load and a quarter of the store instructions)
        if (g.cin == 16 && !qact && !(e.flags & QNN_EPI_NO_LDS16) && qnn_launch_strip16_lds(ms, ep, c.x, w->d_mfma, c.y, c.s) == 0) {
            snprintf(name, name_len, "strip_i4_c16_lds");
            return 0;
        }
        snprintf(name, name_len, g.stride == 2 ? "strip_i4_c%d_s2" : e.proj_x ? "strip_i4_c%d_proj" : "strip_i4_c%d", g.cin);
        if (qnn_launch_strip(g.cin, ms, ep, c.x, w->d_mfma, c.y, c.s) == 0) return 0;
    }
    // small-channel 3x3 int4 layers on the tile kernel (both operands in registers).  Its own shape test: whole 16-pixel
    // tiles, any post-scale, and no in-launch projection shortcut, which exists in the strip kernel only
    const bool small = !e.proj_x && !qact && (g.cin == 16 || g.cin == 32) && g.kh == 3 && g.kw == 3 && g.stride == 1 && g.pt == 1 &&
                       g.pl == 1 && g.pool == 1 && (g.W % 16) == 0 && e.out_store == QNN_STORE_I4 &&
                       (g.cout % (g.cin == 16 ? 16 : 32)) == 0 &&
                       (!e.res || (e.res_store == QNN_STORE_I4 && e.res_cw == e.ocw) ||
                        (e.res_store == QNN_STORE_F32 && e.res_cw == g.cout));
    if (!small || !strip_geom(&ms, g, g.cin / 2, (long)g.N * g.H * g.W, true)) return 1;
    snprintf(name, name_len, "mfma_i4_small_c%d", g.cin);
    return qnn_launch_small(g.cin, ms, es, c.x, w->d_mfma, c.y, c.s);
}
