// Host-side task plan of the row-walking kernels (strip, stem, byte / fixed-point first layer).  Plain C++: no HIP, no
// other header of this library, so the planner is tested on its own (tests/test_strip_plan.py).
//
// The work: every wave walks one 16-pixel column strip (`spr` strips per row) of one image down `rows` rows (pooled
// kernels: row pairs).  An image column is cut into `nch` chunks of `rc` rows, the last one possibly shorter; a task is
// one (image, chunk, strip), and a persistent grid of at most `blocks_cap` workgroups of four waves takes the tasks in
// rounds of 4 * blocks_cap.
//
// Cost model: a round lasts as long as one task, rc rows plus `fill` rows of pipeline fill (ring prologue, filter
// loads), so a plan costs  ceil(N * spr * nch / (4 * blocks_cap)) * (rc + fill).  Short chunks fill the last round
// better, long chunks pay the fill less often; the first candidate with the lowest cost wins.  Candidates:
//   rc_step 1      min(rows, 4) .. rows
//   rc_step 2, 4   rc_step, 2 * rc_step, .. up to rows + rc_step - 1: the kernel wants every chunk to start on a
//                  multiple of rc_step rows (row-pair parity, full four-row store groups)
// `blocks_cap` (what is resident) and `fill` (the pipeline depth) belong to the kernel: each launcher passes its own.
#pragma once

struct StripPlan {
    int spr, nch, rc, ntasks;
    unsigned blocks;            // grid.x: min(ceil(ntasks / 4), blocks_cap)
};

// false: nothing to walk, or more tasks than a kernel's 31-bit task index holds (the launcher reports "not eligible")
inline bool qnn_strip_plan(StripPlan* p, int N, int spr, int rows, int blocks_cap, double fill, int rc_step) {
    if (N < 1 || spr < 1 || rows < 1 || blocks_cap < 1) return false;
    const long nwaves = (long)blocks_cap * 4;
    const int first = rc_step > 1 ? rc_step : rows < 4 ? rows : 4;
    const int last = rc_step > 1 ? rows + rc_step - 1 : rows;
    int best_rc = rows, best_nch = 1;
    double best_cost = 1e300;
    for (int rc = first; rc <= last; rc += rc_step) {
        const int nch = (rows + rc - 1) / rc;
        const long rounds = ((long)N * spr * nch + nwaves - 1) / nwaves;
        const double cost = (double)rounds * (rc + fill);
        if (cost < best_cost) { best_cost = cost; best_rc = rc; best_nch = nch; }
    }
    const long ntasks = (long)N * spr * best_nch;
    if (ntasks >= 2000000000L) return false;
    const long blocks = (ntasks + 3) / 4;
    p->spr = spr; p->nch = best_nch; p->rc = best_rc; p->ntasks = (int)ntasks;
    p->blocks = (unsigned)(blocks < blocks_cap ? blocks : blocks_cap);
    return true;
}

// the six plan arguments every row-walking kernel takes, in the kernels' order (qnn_fastdiv: qnn_common.h)
#define QNN_STRIP_PLAN_ARGS(p) \
    (p).ntasks, (p).spr, qnn_fastdiv((uint32_t)(p).spr), (p).nch, qnn_fastdiv((uint32_t)(p).nch), (p).rc
