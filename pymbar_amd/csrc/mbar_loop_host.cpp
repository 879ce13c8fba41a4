// The host-driven adaptive loop of libmbar_hip.so (pymbar/mbar_solvers.py:575-640): the K x K solve, the candidate construction and
// the convergence test run on the host between the two sweeps.  Used with the host all-reduce transport, for more than 256 states,
// for the non-default kernel variants, and as the continuation when the device-resident loop hands a solve back.
// It reads start -> {pass_a -> candidates -> pass_b -> accept} per iteration: HostLoop owns the state, the methods are the steps.
#include "mbar_ctx.h"

namespace mbar {
namespace host {
namespace {

// MBAR_DEBUG_TIMING: host milliseconds per phase of an iteration, one line per call of the loop.  Inert (no clock is read) unless
// the variable is set.
struct PhaseTimers {
    const bool on = std::getenv("MBAR_DEBUG_TIMING") != nullptr;
    double pass_a = 0, unpack = 0, host = 0, solve = 0, pass_b = 0, t_start = 0;
    double now() const { return on ? now_ms() : 0.0; }
    void start() { t_start = now(); }
    struct Span {  // the time spent in its scope, added to `acc`
        const PhaseTimers& t;
        double& acc;
        const double t0;
        Span(const PhaseTimers& t_, double& acc_) : t(t_), acc(acc_), t0(t_.now()) {}
        ~Span() { acc += t.now() - t0; }
    };
    void print(int64_t nit) const {
        if (on && nit > 0)
            std::fprintf(stderr, "[mbar] adaptive (host loop): %lld it, per it: passA %.3f ms (of it unpacking %.3f), host solve %.3f ms (of it the factorisation + substitutions %.3f), passB %.3f ms, total %.3f ms\n",
                         (long long)nit, pass_a / nit, unpack / nit, host / nit, solve / nit, pass_b / nit, (now_ms() - t_start) / nit);
    }
};

// The choice between the two candidates and the reference's convergence measures, from the candidates and their per-state sums alone.
struct StepVerdict {
    bool take_sci;
    double gn_sci, gn_nr;        // squared gradient norms of the candidates over the sampled states
    double max_delta, max_diff;  // relative change of f, relative distance of the candidates (sampled states except the first)
    bool converged;
};
StepVerdict judge_step(const std::vector<int>& sampled, const std::vector<double>& Nk, const double* f_old, const double* f_sci,
                       const double* f_nr, const double* ps_sci, const double* ps_nr, double tol, bool force_sci) {
    StepVerdict v;
    v.gn_sci = v.gn_nr = 0.0;
    for (int k : sampled) {
        const double a = ps_sci[k] - Nk[k], b = ps_nr[k] - Nk[k];
        v.gn_sci += a * a;
        v.gn_nr += b * b;
    }
    // (every rank holds bit-identical reduced sums, so this choice needs no collective; only the loop exit is agreed on explicitly,
    // because a desynchronised exit would strand the other ranks in an all-reduce)
    // (:607.  A Newton candidate whose gradient is not a number -- a start so poor that H is numerically zero and the
    // step is of order 1e24 -- loses against a finite self-consistent candidate; the reference's comparison would pick
    // it, but the reference's log-space gradient never produces that NaN in the first place)
    v.take_sci = v.gn_sci < v.gn_nr || (std::isnan(v.gn_nr) && !std::isnan(v.gn_sci)) || force_sci;
    const double* f = v.take_sci ? f_sci : f_nr;
    // convergence measures on the sampled states except the first (:627-633)
    const double small = std::min(1e-8, tol);
    v.max_delta = v.max_diff = 0.0;
    bool nan_seen = false;
    for (size_t i = 1; i < sampled.size(); ++i) {
        const int k = sampled[i];
        const double div = std::fabs(f[k]) < small ? 1.0 : std::fabs(f[k]);
        const double d1 = std::fabs(f[k] - f_old[k]) / div, d2 = std::fabs(f_sci[k] - f_nr[k]) / div;
        if (std::isnan(d1)) nan_seen = true;
        v.max_delta = std::max(v.max_delta, d1);
        v.max_diff = std::max(v.max_diff, d2);
    }
    if (nan_seen) v.max_delta = std::numeric_limits<double>::quiet_NaN();
    v.converged = std::isnan(v.max_delta) || (v.max_delta < tol && v.max_diff < std::sqrt(tol));  // :636
    return v;
}

struct HostLoop {
    mbar_ctx* c;
    std::vector<double>& f;     // in / out
    std::vector<double>& psum;  // per-state sums at f
    mbar_solve_result& res;     // carries the counters of the iterations already executed
    double& max_delta;
    const double tol, gamma;
    const int64_t min_sc_iter;
    const int check_convergence;
    double* const history;
    const int64_t history_rows;
    const int64_t K, Kp;
    const int m, first;
    // P mode (257 .. 1024 states, where this loop is the only one): the paneled Gram sweep on u spends 12 row-blocks of exponentials
    // per 32 matrix instructions (0.51-0.55 of the matrix peak).  With a resident probability matrix P = exp(a0 - u - logden(a0))
    // built once at the start point its operands are P_kn / s_n -- ONE multiplication -- with s_n = sum_k P_kn exp(a_k - a0_k) =
    // exp(logden_n(f) - logden_n(a0)) from the log-denominators the evaluation sweep on u leaves anyway; the per-state factors
    // exp(a_k - a0_k) are applied to the K x K result on the host.  One more K x N array; if it does not fit, or a state moves more
    // than 250 kT from the anchor (then: a new anchor), the classic sweep runs.
    bool hp = false;
    GramPlan plan, plan_p;  // Gram sweep on u / on P
    int cur = 0;            // logden slot of the current f
    std::vector<int> pos;   // position of a state among those with samples
    std::vector<double> a0, an_host, cm;  // P mode: aden at the anchor, Kp doubles of scratch, multipliers exp(aden(f) - a0)
    std::vector<double> cand, psum2;      // self-consistent | Newton candidate, and their per-state sums
    std::vector<double> H, g, x;          // Newton system over the sampled states and its solution
    PhaseTimers tm;

    HostLoop(mbar_ctx* c_, std::vector<double>& f_, std::vector<double>& psum_, mbar_solve_result& res_, double& max_delta_, double tol_,
             int64_t min_sc_iter_, double gamma_, int check_convergence_, double* history_, int64_t history_rows_)
        : c(c_), f(f_), psum(psum_), res(res_), max_delta(max_delta_), tol(tol_), gamma(gamma_), min_sc_iter(min_sc_iter_),
          check_convergence(check_convergence_), history(history_), history_rows(history_rows_), K(c_->K), Kp(c_->Kp),
          m((int)c_->sampled.size()), first(c_->sampled[0]), pos((size_t)c_->K, -1), an_host((size_t)c_->Kp), cm((size_t)c_->Kp, 1.0),
          cand(2 * (size_t)c_->K), psum2(2 * (size_t)c_->K), H((size_t)m * m), g(m) {
        for (int i = 0; i < m; ++i) pos[(size_t)c->sampled[i]] = i;
    }
    double* f_sci() { return cand.data(); }
    double* f_nr() { return cand.data() + K; }

    // Initial gradient (mbar_solvers.py:570), the Gram plans and (P mode) the first anchor
    int start() {
        psum.assign(K, 0.0);
        int rc = eval_core(c, f.data(), 1, 0, c->logden[cur], nullptr, psum.data(), nullptr, nullptr);
        if (rc) return rc;
        plan = plan_for(c);
        const bool hp_possible = c->opt_pmode && c->opt_host_pmode && Kp > 256;  // (options: the same on every rank)
        hp = hp_possible && !c->P_failed;
        // ("host_pmode" 2, the default: 256-state panels and 128 x 256 rectangles; 1: the 128-state panels of the sweep on u)
        if (hp) plan_p = c->opt_host_pmode >= 2 ? gram_plan_pmode(Kp) : plan;
        if (hp) {
            rc = anchor_here();
            if (rc) return rc;
        }
        if (hp_possible && c->nranks > 1) {  // a rank whose matrix did not fit must not sweep u while its peers sweep P: the reduced
            bool ok = hp;                    // blocks differ by the per-state factors (and, with the 256-state panels, in number)
            rc = agree_all_ok(c, ok);
            if (rc) return rc;
            hp = ok;
        }
        return MBAR_OK;
    }

    // P at the current f (whose log-denominators are in slot `cur`)
    int anchor_here() {
        if (c->P.grow((size_t)Kp * c->ld) != hipSuccess) {
            (void)hipGetLastError();
            c->P_failed = true;
            hp = false;
            return MBAR_OK;
        }
        HIPCHK(c, c->pm_ld0.grow((size_t)c->ld));
        int rc = need_zeroed_vec(c, c->lden_eff);
        if (rc) return rc;
        a0.assign((size_t)Kp, 0.0);
        build_aden(c, f.data(), a0.data(), Kp);
        std::copy(a0.begin(), a0.end(), c->hstage.p);
        HIPCHK(c, hipMemcpyAsync(d_aden(c), c->hstage, (size_t)Kp * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, launch_make_p(c->stream, c->num_cu, c->u, c->ld, c->N, Kp, d_aden(c), c->logden[cur], c->P));
        HIPCHK(c, hipMemcpyAsync(c->pm_ld0, c->logden[cur], (size_t)c->N * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));  // (hstage is re-used below)
        c->P_valid = false;  // (not the device-resident loop's warm-start matrix)
        return MBAR_OK;
    }

    // Pass A: Gram at f with the known logden -> H = -Gram over the sampled states (mbar_solvers.py:581; + diag in candidates)
    int pass_a() {
        PhaseTimers::Span span(tm, tm.pass_a);
        const GramPlan& pl = hp ? plan_p : plan;
        const size_t total = pl.total_blocks * 256;
        int rc = ensure_red(c, total);
        if (!rc) rc = reserve_gram(c, pl, hp);  // (what is queued below before run_gram must not see the buffers replaced)
        if (rc) return rc;
        std::vector<double> an((size_t)Kp);
        build_aden(c, f.data(), an.data(), Kp);
        if (hp) {  // multipliers relative to the anchor; a state that has moved too far re-anchors P at the current f
            bool far = false;
            for (int64_t k = 0; k < Kp; ++k) {
                const bool live = !std::isinf(an[k]) && !std::isinf(a0[k]);
                const double d = live ? an[k] - a0[k] : 0.0;
                if (!(std::fabs(d) < 250.0) || std::isinf(an[k]) != std::isinf(a0[k])) far = true;
                cm[k] = live ? std::exp(d) : 0.0;
            }
            if (far) {
                rc = anchor_here();
                if (rc) return rc;
                for (int64_t k = 0; k < Kp; ++k) cm[k] = std::isinf(a0[k]) ? 0.0 : 1.0;
            }
        }
        if (hp) {
            HIPCHK(c, launch_rinv_from_logden(c->stream, c->pm_ld0, c->logden[cur], c->cw, c->weighted, c->N, c->lden_eff));
            rc = run_gram(c, d_anum(c), c->lden_eff, 0, pl, c->P);
        } else {
            std::copy(an.begin(), an.end(), c->hstage + 2 * Kp);
            HIPCHK(c, hipMemcpyAsync(d_anum(c), c->hstage + 2 * Kp, an.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
            rc = run_gram(c, d_anum(c), c->logden[cur], 0, pl);
        }
        if (rc) return rc;
        rc = fetch_red(c, total);
        if (rc) return rc;
        PhaseTimers::Span unpack(tm, tm.unpack);
        // (with the per-state factors the P-mode sweep leaves out; m x m over the sampled states)
        unpack_gram_to_hessian(pl, c->hred, K, hp ? cm.data() : nullptr, pos.data(), m, H.data(), host_team_size(m));
        return MBAR_OK;
    }

    // Both candidates: the Newton step (:582-584) and the self-consistent update (:587-588)
    int candidates() {
        PhaseTimers::Span span(tm, tm.host);
        for (int i = 0; i < m; ++i) {
            const int ki = c->sampled[i];
            g[i] = psum[ki] - c->Nk[ki];
            H[(size_t)i * m + i] += psum[ki];
        }
        {
            PhaseTimers::Span solve(tm, tm.solve);
            newton_direction(H, g, m, x);  // :582-583
        }
        std::copy(f.begin(), f.end(), f_sci());
        std::copy(f.begin(), f.end(), f_nr());
        bool underflow = false;
        for (int i = 0; i < m; ++i) {
            const int k = c->sampled[i];
            f_nr()[k] = f[k] - gamma * x[i];                   // :584
            f_sci()[k] = f[k] - std::log(psum[k] / c->Nk[k]);  // :587 via s_k
            if (!(psum[k] > 1e-290)) underflow = true;
        }
        if (underflow) {
            // A state whose weights at the current f are below the fp64 range (a start more than ~700 kT from the answer):
            // its sum p underflowed, the reference's log-space update (:240-241) does not.  Take that path for this
            // iteration: the all-state log-space reduction (two more sweeps; slot 0 holds logden(f) again or is about
            // to be overwritten by pass B anyway).
            std::vector<double> ln((size_t)K);
            int rc = mbar_lognum(c, f.data(), ln.data());
            if (rc) return rc;
            for (int i = 0; i < m; ++i) f_sci()[c->sampled[i]] = -ln[(size_t)c->sampled[i]];
        }
        const double shift = f_sci()[first];
        for (int i = 0; i < m; ++i) f_sci()[c->sampled[i]] -= shift;  // :588
        return MBAR_OK;
    }

    // Pass B on the same matrix: an element of candidate 0 is P_kn exp(a_k - a0_k) -- one multiplication, no exponential, no
    // shared shift (the eight waves of a workgroup meet once per tile instead of twice) -- and logden_n = logden_n(a0) + log(sum).
    // `used` stays false (the classic sweep on u runs) when a candidate is not finite or outside the 250 kT window of the anchor.
    int pass_b_on_p(double* ldA, double* ldB, bool& used) {
        used = false;
        if (!hp || !split_sweep_ok(c, Kp) || c->u_poison) return MBAR_OK;
        std::vector<double> h((size_t)2 * Kp, 0.0), a1((size_t)Kp);
        build_aden(c, f_sci(), an_host.data(), Kp);
        build_aden(c, f_nr(), a1.data(), Kp);
        for (int64_t k = 0; k < Kp; ++k) {
            if (std::isinf(a0[k])) {  // a state without samples (or padding): no element
                if (!std::isinf(an_host[k]) || !std::isinf(a1[k])) return MBAR_OK;
                continue;
            }
            const double d0 = an_host[k] - a0[k], d1 = a1[k] - an_host[k];
            if (!(std::fabs(d0) < 250.0) || !(std::fabs(d1) < 300.0)) return MBAR_OK;
            h[(size_t)k] = std::exp(d0);
            h[(size_t)Kp + k] = std::exp(d1);
        }
        const size_t n_ps = (size_t)2 * Kp, total = n_ps + 2;
        int rc = ensure_red(c, total);
        if (!rc) rc = ensure(c, c->part, (size_t)c->num_cu * 2 * (Kp + 1));
        if (!rc) rc = ensure(c, c->scratch, (size_t)(c->num_cu / 32 + 2) * 2 * (Kp + 1));
        if (rc) return rc;
        std::copy(h.begin(), h.end(), c->hstage.p);
        HIPCHK(c, hipMemcpyAsync(d_aden(c), c->hstage, h.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
        if (ldA == c->logden[0] || ldB == c->logden[0]) c->ld0_valid = false;
        int blocks = 0;
        double* obj_part = c->part + (size_t)c->num_cu * 2 * Kp;
        {
            ScopedTimer t(c, MBAR_TIMER_LSE);
            HIPCHK(c, launch_lse_split(c->stream, c->num_cu, 2, c->P, c->ld, c->N, Kp, d_aden(c), c->cw, ldA, ldB, nullptr, c->part, obj_part,
                                       &blocks, c->pm_ld0));
        }
        {
            ScopedTimer t(c, MBAR_TIMER_REDUCE);
            HIPCHK(c, launch_reduce(c->stream, c->part, blocks, (int64_t)n_ps, c->scratch, c->red));
            HIPCHK(c, launch_reduce(c->stream, obj_part, blocks, 2, c->scratch, c->red + n_ps));
        }
        rc = fetch_red(c, total);
        if (rc) return rc;
        for (int64_t k = 0; k < K; ++k) {
            psum2[k] = c->hred[(size_t)k];
            psum2[(size_t)K + k] = c->hred[(size_t)Kp + k] * h[(size_t)Kp + k];  // (the second candidate's sums come without its ratio)
        }
        used = true;
        return MBAR_OK;
    }

    // Pass B: both candidates in one sweep (:589-594), their log-denominators into the two slots `cur` does not name
    int pass_b() {
        PhaseTimers::Span span(tm, tm.pass_b);
        double* ldA = c->logden[(cur + 1) % 3];
        double* ldB = c->logden[(cur + 2) % 3];
        bool on_p = false;
        int rc = pass_b_on_p(ldA, ldB, on_p);
        if (!rc && !on_p) rc = eval_core(c, cand.data(), 2, 0, ldA, ldB, psum2.data(), nullptr, nullptr);
        return rc;
    }

    // The better candidate becomes f (:607), the counters and the history row of iteration `it`; `done`: converged, on every rank
    int accept(int64_t it, bool& done) {
        const StepVerdict v = judge_step(c->sampled, c->Nk, f.data(), f_sci(), f_nr(), psum2.data(), psum2.data() + K, tol,
                                         res.sci_iter < min_sc_iter);
        const size_t off = v.take_sci ? 0 : (size_t)K;
        std::copy(cand.begin() + off, cand.begin() + off + K, f.begin());
        std::copy(psum2.begin() + off, psum2.begin() + off + K, psum.begin());
        cur = (cur + (v.take_sci ? 1 : 2)) % 3;
        (v.take_sci ? res.sci_iter : res.nr_iter)++;
        max_delta = v.max_delta;
        res.iterations = it + 1;
        res.gram_sweeps += 1;
        if (history && it < history_rows) {
            history[4 * it + 0] = v.take_sci ? 0 : 1;
            history[4 * it + 1] = std::sqrt(v.gn_sci);
            history[4 * it + 2] = std::sqrt(v.gn_nr);
            history[4 * it + 3] = max_delta;
        }
        double stop = (check_convergence && v.converged) ? 1.0 : 0.0;
        if (check_convergence) {
            int rc = agree_with_rank0(c, &stop, 1);
            if (rc) return rc;
        }
        done = stop > 0.5;
        if (done) res.success = 1;
        return MBAR_OK;
    }

    int run(int64_t maxiter) {
        const int64_t it0 = res.iterations;
        tm.start();
        bool done = false;
        for (int64_t it = it0; it < maxiter && !done; ++it) {
            int rc = pass_a();
            if (!rc) rc = candidates();
            if (!rc) rc = pass_b();
            if (!rc) rc = accept(it, done);
            if (rc) return rc;
        }
        tm.print(res.iterations - it0);
        return MBAR_OK;
    }
};

}  // namespace

// `res` carries the counters of the iterations already executed; `f` in/out; psum at the returned f in `psum`.
int adaptive_host_loop(mbar_ctx* c, std::vector<double>& f, double tol, int64_t maxiter, int64_t min_sc_iter, double gamma,
                       int check_convergence, double* history, int64_t history_rows, mbar_solve_result& res,
                       std::vector<double>& psum, double& max_delta) {
    HostLoop loop(c, f, psum, res, max_delta, tol, min_sc_iter, gamma, check_convergence, history, history_rows);
    int rc = loop.start();
    return rc ? rc : loop.run(maxiter);
}

}  // namespace host
}  // namespace mbar
