// ---- BAR root find (mbar_k_bar.hip; C ABI in mbar_bar.cpp) ---------------------------------------------------------------------
#pragma once
#include "mbar_common.h"

namespace mbar {

// The reference's bracket / false-position / bisection / self-consistent loop (pymbar other_estimators.bar) as a resumable state
// machine: each call consumes F at the previous requests and either issues the next requests (nreq = 1 or 2) or ends (status != 0).
// The same function runs in the step kernel and in mbar_bar_step_host.  Contraction is off so that every operation is the one
// IEEE operation of the reference's Python floats (no fma), in the reference's order.
enum : int64_t { BAR_RUNNING = 0, BAR_DONE = 1, BAR_NAN_BRACKET = 2, BAR_BOUNDS = 3, BAR_NOT_CONVERGED = 4 };
enum : int64_t { BAR_FALSE_POSITION = 0, BAR_BISECTION = 1, BAR_SELF_CONSISTENT = 2 };
enum : int64_t { BAR_PH_INIT = 0, BAR_PH_BRACKET0 = 1, BAR_PH_WIDEN = 2, BAR_PH_LOOP = 3 };

MBAR_HD inline void bar_finish_loop(mbar_bar_state& s, bool broke) {
    // after `for iteration in range(maximum_iterations + 1)`: iteration holds the last value whether the loop broke or not
    if (!broke) s.iteration = s.maximum_iterations;
    s.nreq = 0;
    s.status = (s.iterated && !(s.iteration < s.maximum_iterations)) ? BAR_NOT_CONVERGED : BAR_DONE;
}

MBAR_HD inline int64_t bar_advance(mbar_bar_state& s, const double* F) {
#pragma clang fp contract(off)
    if (s.status != BAR_RUNNING) return s.status;
    const bool bracketed = s.method != BAR_SELF_CONSISTENT;
    switch (s.phase) {
    case BAR_PH_INIT:
        s.DeltaF_initial = s.DeltaF;
        s.iteration = 0;
        s.nzero = 0;
        if (bracketed) {
            s.req[0] = s.UpperB;
            s.req[1] = s.LowerB;
            s.nreq = 2;
            s.phase = BAR_PH_BRACKET0;
            return s.status;
        }
        break;  // to the loop, iteration 0
    case BAR_PH_BRACKET0:
    case BAR_PH_WIDEN: {
        s.FUpperB = F[0];
        s.FLowerB = F[1];
        s.nzero += 2;
        if (s.phase == BAR_PH_BRACKET0 && (s.FUpperB != s.FUpperB || s.FLowerB != s.FLowerB)) {
            s.DeltaF = 0.0;
            s.nreq = 0;
            s.status = BAR_NAN_BRACKET;
            return s.status;
        }
        if (s.FUpperB * s.FLowerB > 0) {
            // widen: max(abs(.), 0.1) keeps its first argument unless 0.1 is larger (Python's max)
            const double FAve = (s.UpperB + s.LowerB) / 2;
            const double du = fabs(s.UpperB - FAve), dl = fabs(s.LowerB - FAve);
            s.UpperB = s.UpperB - (0.1 > du ? 0.1 : du);
            s.LowerB = s.LowerB + (0.1 > dl ? 0.1 : dl);
            s.req[0] = s.UpperB;
            s.req[1] = s.LowerB;
            s.nreq = 2;
            s.phase = BAR_PH_WIDEN;
            return s.status;
        }
        break;  // to the loop, iteration 0
    }
    case BAR_PH_LOOP: {
        // the body of one iteration after its evaluation
        s.nzero += 1;
        if (s.method == BAR_SELF_CONSISTENT) s.DeltaF = -F[0] + s.DeltaF;
        else s.FNew = F[0];
        if (s.method == BAR_FALSE_POSITION && s.FNew == 0) {
            s.relative_change = 1e-15;
            bar_finish_loop(s, true);
            return s.status;
        }
        goto check;
    }
    default:
        s.status = BAR_BOUNDS;
        return s.status;
    }
    // top of the loop at s.iteration
    for (;;) {
        s.DeltaF_old = s.DeltaF;
        if (s.method == BAR_FALSE_POSITION) {
            if (s.LowerB == 0.0 && s.UpperB == 0.0) {
                // no evaluation: FNew = 0 ends the loop
                s.DeltaF = 0.0;
                s.FNew = 0.0;
                s.relative_change = 1e-15;
                bar_finish_loop(s, true);
                return s.status;
            }
            s.DeltaF = s.UpperB - s.FUpperB * (s.UpperB - s.LowerB) / (s.FUpperB - s.FLowerB);
        } else if (s.method == BAR_BISECTION) {
            s.DeltaF = (s.UpperB + s.LowerB) / 2;
        }
        s.req[0] = s.DeltaF;
        s.nreq = 1;
        s.phase = BAR_PH_LOOP;
        return s.status;
    check:
        if (s.DeltaF == 0.0) {
            bar_finish_loop(s, true);
            return s.status;
        }
        if (s.iterated) {
            s.relative_change = fabs((s.DeltaF - s.DeltaF_old) / s.DeltaF);
            if (s.iteration > 0 && s.relative_change < s.relative_tolerance) {
                bar_finish_loop(s, true);
                return s.status;
            }
        }
        if (bracketed) {
            if (s.FUpperB * s.FNew < 0) {
                s.LowerB = s.DeltaF;
                s.FLowerB = s.FNew;
            } else if (s.FLowerB * s.FNew <= 0) {
                s.UpperB = s.DeltaF;
                s.FUpperB = s.FNew;
            } else {
                s.nreq = 0;
                s.status = BAR_BOUNDS;
                return s.status;
            }
        }
        if (s.iteration == s.maximum_iterations) {
            bar_finish_loop(s, false);
            return s.status;
        }
        s.iteration += 1;
    }
}

// Device side.  Values of every side are cut into chunks of MBAR_BAR_CHUNK (chunk c: side seg[c] = 2 p + (0 F, 1 R), values
// [start[c], start[c] + len[c]) of w, minimum wmin[c]); the chunks of one side are consecutive, cbeg[s] .. cbeg[s + 1].
constexpr int BAR_WG = 256;
constexpr int BAR_PER_THREAD = MBAR_BAR_CHUNK / BAR_WG;
struct BarData {
    const double* w;
    const int64_t* start;
    const int* len;
    const int* seg;
    const double* wmin;      // [nchunks] minimum of the chunk (+inf: every value is +inf)
    const int64_t* cbeg;     // [2 P + 1]
    const double* M;         // [P] log(n_F / n_R)
    int64_t P, nchunks;
};
// partial of a chunk at one DeltaF: the shift (hi + lo, -inf for a chunk of +inf values) and the sums of the shifted factors and
// of their squares
struct BarPartial {
    double hi, lo, s1, s2;
};
// evaluation pass: every chunk of every problem still running, at its requests; part[(r * nchunks) + c]
hipError_t launch_bar_eval(hipStream_t st, const BarData& d, const mbar_bar_state* states, BarPartial* part);
// merge of the partials and one step of every running state (advance != 0), or (advance == 0) out[p][5] of the first request
hipError_t launch_bar_step(hipStream_t st, const BarData& d, mbar_bar_state* states, const BarPartial* part, int advance,
                           double* out, int* status);
// one-sided moments of every side: out[s][5] (include/mbar_hip.h, mbar_bar_moments); scratch: [3][nchunks]
hipError_t launch_bar_moments(hipStream_t st, const BarData& d, const int64_t* nside, double* scratch, double* out);

}  // namespace mbar
