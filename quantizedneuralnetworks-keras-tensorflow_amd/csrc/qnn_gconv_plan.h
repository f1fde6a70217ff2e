// Tile arithmetic of the matrix-pipe form of the grouped convolution (include/qnn_abi_gconv.h, k_gc_mfma in
// qnn_gconv.hip).  Plain C++ without HIP types: prepack, the route rule and the launcher use it, and
// tests/test_gconv_plan.py compiles it on its own.  THE one place the rule lives; the header states it and
// tests/gconv_cases.py restates it.
//
// Cg = Cin / groups input channels and Fg = Cout / groups filters per group.  A TILE is 16 consecutive filters
// 16 T .. 16 T + 15.  In NHWC it reads one contiguous run of R input channels starting at channel c0:
//   Fg % 16 == 0   the tile lies in group 16 T / Fg:           t = 1,       R = Cg,     c0 = (16 T / Fg) * Cg;
//   16 % Fg == 0   the tile covers the t = 16 / Fg groups t T .. t T + t - 1:  R = t Cg,  c0 = T * R
//                  (the weights are block-diagonal inside the tile: filter f meets only its own group's Cg channels).
// The K = 64 of one v_mfma_i32_16x16x64_i8 is four SLOTS of 16 channels, one per lane quad.  The slots of a tile are the
// (tap, 16-channel chunk of the run) pairs, tap-major: slot s = tap * (R / 16) + chunk, tap = ky * kw + kx.  K-step k
// holds slots 4 k .. 4 k + 3; the slots beyond the last real one (only in the last step) are PADDING: zero weight bytes
// and an out-of-range load offset.
#pragma once
#include <stddef.h>
#include <stdint.h>

#define QNN_GC_MAX_RUN 16384   // R <= 16384 channels

#ifdef __HIPCC__
#define QNN_GC_HD __host__ __device__
#else
#define QNN_GC_HD
#endif

struct GcPlan {
    int Cg, Fg;      // channels / filters per group
    int t;           // groups per tile
    int R;           // channels a tile reads
    int spt;         // slots per tap = R / 16
    int slots;       // kh * kw * spt
    int steps;       // K-steps = ceil(slots / 4)
    int tiles;       // Cout / 16
};

// The shape half of the eligibility rule; fills *p when it holds.  All arguments >= 1, Cin and Cout multiples of groups.
QNN_GC_HD static inline bool qnn_gc_plan(GcPlan* p, int kh, int kw, int cin, int cout, int groups) {
    const int Cg = cin / groups, Fg = cout / groups;
    if (cout % 16 != 0) return false;
    if (Fg % 16 != 0 && 16 % Fg != 0) return false;
    const int t = Fg % 16 == 0 ? 1 : 16 / Fg;
    const long long R = (long long)t * Cg;
    if (R % 16 != 0 || R > QNN_GC_MAX_RUN) return false;
    p->Cg = Cg; p->Fg = Fg; p->t = t; p->R = (int)R;
    p->spt = (int)R / 16;
    p->slots = kh * kw * p->spt;
    p->steps = (p->slots + 3) / 4;
    p->tiles = cout / 16;
    // the operand image, 1024 bytes per (tile, K-step), stays below 2^31 bytes
    return (long long)p->tiles * p->steps * 1024 < (1LL << 31);
}

// first input channel of tile T's run (a multiple of 16)
QNN_GC_HD static inline int qnn_gc_tile_channel(const GcPlan* p, int tile) {
    return p->t == 1 ? (16 * tile / p->Fg) * p->Cg : tile * p->R;
}

// what slot s of a tile holds: true and (tap, chunk) for a real slot, false for a padding slot
QNN_GC_HD static inline bool qnn_gc_slot(const GcPlan* p, int s, int* tap, int* chunk) {
    if (s < 0 || s >= p->slots) return false;
    *tap = s / p->spt;
    *chunk = s - *tap * p->spt;
    return true;
}

// THE route rule of the matrix-pipe form: the stores, the shape (qnn_gc_plan), both pointers 16-byte aligned, one input
// image as stored below 2^31 bytes.  The handle's half is asked at prepack with the pointers 0 and img_bytes 0.
static inline bool qnn_gc_mfma_ok(GcPlan* p, int store, int x_store, int out_store, int kh, int kw, int cin, int cout,
                                  int groups, uintptr_t x, uintptr_t y, size_t img_bytes) {
    if ((store != 4 && store != 8) || x_store != store || out_store != x_store) return false;      // QNN_STORE_I4 / _I8
    if (!qnn_gc_plan(p, kh, kw, cin, cout, groups)) return false;
    if (x % 16 != 0 || y % 16 != 0) return false;
    return img_bytes < ((size_t)1 << 31);
}
