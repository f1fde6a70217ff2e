// Host plan of the register-fed dense GEMM (k_dense_mfma, qnn_dense_mfma.hip): how many unit tiles a wave takes (NT) and
// over how many of a workgroup's four waves K is split (ks).  Plain C++ without HIP types: the route uses it, and
// tests/test_dense_plan.py compiles it on its own.  THE one place the rule lives; tests/dense_mfma_cases.py restates it.
//
// N images x `units` outputs over `steps` K-steps are
//     blocks = ceil(units / (16 nt)) * ceil(ceil(N / 16) / (4 / ks))
// workgroups, of which `cus` * kDenseResident run at a time.  Cost model, in K-steps of one wave: a round lasts
// ceil(steps / ks) * (nt + 1) + kDenseFill (+ kDenseMeet when ks > 1): nt matrix operations and nt + 1 operand loads per
// K-step, the pipeline fill and the epilogue once, and the trip through LDS where K is split.  A plan costs rounds * that;
// candidates are tried from the widest tile and the smallest split, the first with the lowest cost wins.  Few rows and a
// long K therefore split K four ways (64 x 1024 -> 1024: NT 1, ks 4, one workgroup per CU); a batch that fills the chip on
// its own keeps K whole and takes the widest tile, which loads the fewest operands per matrix operation (4096 images:
// NT 4, ks 1 at K = 64 and at K = 8192).
#pragma once
#include <stddef.h>
#include <stdint.h>

constexpr int kDenseResident = 4;   // workgroups per CU: one wave on each SIMD, four deep
constexpr int kDenseFill = 8, kDenseMeet = 2;

struct DensePlan {
    int nt, ks;                 // unit tiles per wave (1, 2, 4), waves along K (1, 2, 4)
    int ublocks;                // workgroups along the units; workgroup b is (unit block b % ublocks, image group b / ublocks)
    unsigned blocks;            // grid.x
};

// false: nothing to compute, or more workgroups than a grid's x extent holds (the route declines)
static inline bool dense_plan(DensePlan* p, long N, int units, int steps, int cus) {
    if (N < 1 || units < 16 || steps < 1 || cus < 1) return false;
    const long itiles = (N + 15) / 16, utiles = (units + 15) / 16, cap = (long)cus * kDenseResident;
    double best = 1e300;
    for (int nt = 4; nt >= 1; nt >>= 1)
        for (int ks = 1; ks <= 4; ks <<= 1) {
            const long ub = (utiles + nt - 1) / nt, per = 4 / ks;
            const long blocks = ub * ((itiles + per - 1) / per);
            const long walk = (long)((steps + ks - 1) / ks) * (nt + 1) + kDenseFill + (ks > 1 ? kDenseMeet : 0);
            const double cost = (double)((blocks + cap - 1) / cap) * (double)walk;
            if (cost < best && blocks < 2147483648L) {
                best = cost;
                p->nt = nt; p->ks = ks; p->ublocks = (int)ub; p->blocks = (unsigned)blocks;
            }
        }
    return best < 1e300;
}
