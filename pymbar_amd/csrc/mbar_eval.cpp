// Host side of libmbar_hip.so, the evaluation engine (mbar_ctx.h lists the files of the context layer): the sweeps and their
// reductions (run_lse, the Gram plans, run_gram), what turns reduced blocks into matrices, eval_core, and the evaluation entry
// points of the C ABI built on them.  Drives the gfx950 kernels of mbar_k_*.hip on the device-resident shard of u_kn.
#include "mbar_ctx.h"

#include <cassert>

using namespace mbar;
using namespace mbar::host;

namespace mbar {
namespace host {

bool f_is_finite(const mbar_ctx* c, const double* f, int nf) {
    for (int i = 0; i < nf; ++i)
        for (int64_t k = 0; k < c->K; ++k)
            if (c->Nk[k] > 0.0 && !std::isfinite(f[(size_t)i * c->K + k])) return false;
    return true;
}

// ---- evaluation building blocks -----------------------------------------------------------------
// Which specialised evaluation kernels this context qualifies for (flags for lse_geometry).  Row pitches from 7.6e7 samples up
// need 64-bit lane offsets in the tile DMA; only the general kernels are instantiated for that.
bool wide_pitch(const mbar_ctx* c) { return (uint64_t)c->ld * 56u + 128u >= (1ull << 32); }
int lse_variant_for(const mbar_ctx* c) {
    if (wide_pitch(c)) return 0;
    int v = 0;
    // bit 4: the context qualifies for the few-state kernel (one sample per lane, 64-sample tiles); lse_geometry
    // takes it for single-candidate sweeps of up to 32 states
    if (c->opt_small && c->Kp <= 32 && c->ld % 64 == 0) v |= 0x10;
    // bit 5: wide panels (129..256 states) may use the single-buffer kernel (four waves per CU instead of two)
    if (c->opt_wide && c->Kp > 128) v |= 0x20;
    return v;
}
bool use_fast(const mbar_ctx* c) { return c->K <= MAX_FAST_K && !c->opt_force_generic; }

// Host vector a[k] = f[k] + ln N_k (-inf where N_k = 0 or k >= K), written into out[rows].
void build_aden(const mbar_ctx* c, const double* f, double* out, int64_t rows) {
    const double ninf = -std::numeric_limits<double>::infinity();
    for (int64_t k = 0; k < rows; ++k) out[k] = (k < c->K && c->Nk[k] > 0.0) ? f[k] + c->lnNk[k] : ninf;
}

// 257 .. 1024 states: the one-read evaluation kernel whose eight waves split the rows of a tile
bool split_sweep_ok(const mbar_ctx* c, int64_t rows) {
    return !use_fast(c) && !c->opt_force_generic && !wide_pitch(c) && rows <= 1024 && rows % 64 == 0 && c->opt_wide;
}

// What run_lse needs of part and scratch for nf candidates, and (fast path) its launch geometry
static RecordNeed lse_need(const mbar_ctx* c, int nf, int64_t rows, LaunchGeom* g) {
    RecordNeed need;
    if (use_fast(c)) {
        *g = lse_geometry((int)(rows / 16), nf, c->num_cu, (c->N + TS - 1) / TS, c->opt_grid, lse_variant_for(c));
        g->balanced = c->opt_small_balanced ? 1 : 0;
        need.add(g->nwaves, (size_t)nf * rows + nf);
    } else if (split_sweep_ok(c, rows)) {
        need = {(size_t)c->num_cu * nf * (rows + 1), (size_t)(c->num_cu / 32 + 2) * nf * (rows + 1)};
    } else {
        need = {(size_t)c->num_cu * 8 + (size_t)512 * c->K, (size_t)64 * (c->K + 8)};
    }
    return need;
}

// Evaluation pass for nf vectors whose aden already sits in d_aden (device, row pitch `rows`).
// Results: red[0 .. nf*rows) = psum, red[nf*rows .. nf*rows+nf) = sum logden.  Not all-reduced.
// (Sizes part and scratch itself; a caller that queues anything first -- eval_core: the copy of aden -- has sized them already.)
int run_lse(mbar_ctx* c, int nf, int64_t rows, double* ld0, double* ld1, bool use_offset) {
    const double* dn = use_offset ? c->dn : nullptr;
    const bool fast = use_fast(c), split = !fast && split_sweep_ok(c, rows);
    const size_t rec = (size_t)nf * rows;
    LaunchGeom g{};
    int rc = reserve(c, lse_need(c, nf, rows, &g));
    if (rc) return rc;
    if (fast) {
        const int nb = (int)(rows / 16);
        double* psum_part = c->part;
        double* obj_part = c->part + (size_t)g.nwaves * rec;
        {
            ScopedTimer t(c, MBAR_TIMER_LSE);
            HIPCHK(c, launch_lse(c->stream, nb, nf, g, c->u, c->ld, c->N, d_aden(c), c->cw, ld0,
                                 ld1, dn, psum_part, obj_part));
        }
        {
            // (per-state sums and objective terms in ONE pair of launches: at small sizes an evaluation is its launches -- the
            // scipy-driven protocol stages call this thirty times per solve)
            ScopedTimer t(c, MBAR_TIMER_REDUCE);
            HIPCHK(c, launch_reduce2(c->stream, psum_part, (int64_t)rec, obj_part, nf, g.nwaves, c->scratch, c->red, c->red + rec));
        }
        return MBAR_OK;
    }
    // 257 .. 1024 states: the rows of a tile split over the eight waves of a workgroup -- ONE read of the matrix for one or
    // two candidates (the second through its ratio row, like the narrower kernels; the layout-agnostic kernels below read the
    // matrix twice per candidate: log-sum-exp pass + column-sum pass)
    if (split) {
        int blocks = 0;
        double* obj_part = c->part + (size_t)c->num_cu * nf * rows;
        {
            ScopedTimer t(c, MBAR_TIMER_LSE);
            HIPCHK(c, launch_lse_split(c->stream, c->num_cu, nf, c->u, c->ld, c->N, rows, d_aden(c), c->cw, ld0, nf == 2 ? ld1 : nullptr, dn,
                                       c->part, obj_part, &blocks));
        }
        ScopedTimer t(c, MBAR_TIMER_REDUCE);
        HIPCHK(c, launch_reduce(c->stream, c->part, blocks, (int64_t)nf * rows, c->scratch, c->red));
        HIPCHK(c, launch_reduce(c->stream, obj_part, blocks, nf, c->scratch, c->red + (size_t)nf * rows));
        return MBAR_OK;
    }
    // generic: one f at a time
    for (int i = 0; i < nf; ++i) {
        int blocks = 0, cblocks = 0;
        double* ldst = i == 0 ? ld0 : ld1;
        if (!ldst) ldst = c->logden[i];  // the column-sum kernel needs logden even if the caller does not
        {
            ScopedTimer t(c, MBAR_TIMER_LSE);
            HIPCHK(c, launch_lse_generic(c->stream, c->num_cu, c->u, c->ld, c->N, c->K, d_aden(c) + i * rows, c->cw,
                                         ldst, dn, c->part, &blocks));
        }
        {
            ScopedTimer t(c, MBAR_TIMER_REDUCE);
            HIPCHK(c, launch_reduce(c->stream, c->part, blocks, 1, c->scratch, c->red + nf * rows + i));
        }
        {
            ScopedTimer t(c, MBAR_TIMER_LSE);
            HIPCHK(c, launch_colsum_generic(c->stream, c->num_cu, c->u, c->ld, c->N, c->K, d_aden(c) + i * rows, c->cw,
                                            ldst, c->part, &cblocks));
        }
        {
            ScopedTimer t(c, MBAR_TIMER_REDUCE);
            HIPCHK(c, hipMemsetAsync(c->red + i * rows, 0, rows * sizeof(double), c->stream));
            HIPCHK(c, launch_reduce(c->stream, c->part, cblocks, c->K, c->scratch, c->red + i * rows));
        }
    }
    return MBAR_OK;
}

// Shared by the two plans below: Kp (a multiple of 64 wherever there is more than one panel) split into panels of `width`
// states and a shorter last one; the panels' diagonal items (upper-triangular blocks, one launch each) open the plan
struct Panel { int64_t r0; int nb; };
static std::vector<Panel> diag_panels(int64_t Kp, int width, GramPlan& p) {
    std::vector<Panel> panels;
    for (int64_t r = 0; r < Kp;) {
        const int nb = Kp - r >= width ? width / 16 : (int)((Kp - r) / 16);
        panels.push_back({r, nb});
        r += 16 * nb;
    }
    for (const auto& a : panels) {
        const int nblk = a.nb * (a.nb + 1) / 2;
        p.items.push_back({true, a.r0, a.r0, a.nb, a.nb, nblk, p.total_blocks});
        p.total_blocks += nblk;
    }
    return panels;
}
static void add_rect(GramPlan& p, int64_t ri, int64_t rj, int nbi, int nbj) {
    p.items.push_back({false, ri, rj, nbi, nbj, nbi * nbj, p.total_blocks});
    p.total_blocks += (size_t)nbi * nbj;
}

// Gram-pass geometry: list of launches and where their 16 x 16 blocks land.  Up to 128 states: one diagonal panel.
// Beyond: 128-state panels (+ one trailing 64-state panel); a diagonal panel is one launch (upper-triangular blocks),
// a pair of panels is covered by 64 x 128 rectangles (nbi = 4 block rows of the I panel x nbj = 8 block columns of the
// J panel = 32 blocks, the most one wave's register file holds next to the operands).
GramPlan gram_plan(int64_t Kp, bool quad) {
    GramPlan p;
    // (quad: 129 .. 256 states as ONE panel, its blocks split over the four waves of a workgroup)
    const std::vector<Panel> panels = diag_panels(Kp, Kp <= 128 || quad ? (int)Kp : 128, p);
    // beyond 128 states padded_K gives multiples of 64: every panel has 128 states but the last, which may have 64
    for (size_t ia = 0; ia < panels.size(); ++ia)
        for (size_t ib = ia + 1; ib < panels.size(); ++ib) {
            const Panel &a = panels[ia], &b = panels[ib];
            if (b.nb == 8) {  // 128 x 128: two 64 x 128 rectangles
                for (int h = 0; h < 2; ++h) add_rect(p, a.r0 + 64 * h, b.r0, 4, 8);
            } else {  // the trailing 64-state panel against a 128-state one: I = the short panel
                assert(b.nb == 4 && "gram_plan: beyond 128 states Kp must be a multiple of 64");
                add_rect(p, b.r0, a.r0, 4, 8);
            }
        }
    return p;
}

// The plan of the host-driven loop's P mode (more than 256 states): 256-state panels, each ONE read of its rows (k_gram_quad on
// the probability matrix), the remainder (64 / 128 / 192 states) as one more diagonal panel, and between the panels the
// rectangles of k_gram_rect: 128 x 256 (64 x 256 for the short remainder), four waves on one shared tile stream.  At 1024 states
// 4 + 12 launches that read 5632 rows of the matrix (gram_plan above: 64 launches, 11776 rows).
GramPlan gram_plan_pmode(int64_t Kp) {
    GramPlan p;
    const std::vector<Panel> panels = diag_panels(Kp, 256, p);
    for (size_t ia = 0; ia < panels.size(); ++ia)
        for (size_t ib = ia + 1; ib < panels.size(); ++ib) {
            const Panel &a = panels[ia], &b = panels[ib];  // a is a 256-state panel; b one too, or the remainder
            const Panel &rows = b.nb == 16 ? a : b, &cols = b.nb == 16 ? b : a;
            for (int done = 0; done < rows.nb;) {
                const int nbi = rows.nb - done >= 8 ? 8 : 4;
                add_rect(p, rows.r0 + 16 * done, cols.r0, nbi, 16);
                done += nbi;
            }
        }
    return p;
}

// 129 .. 256 states: the one-read kernel (k_gram_quad) needs LDS-DMA staging
bool use_quad(const mbar_ctx* c) { return c->opt_quad && use_fast(c) && c->Kp > 128 && c->Kp <= 256; }
GramPlan plan_for(const mbar_ctx* c) { return gram_plan(c->Kp, use_quad(c)); }
// blocks of 16 states of the 192- / 256-row panel that hold real states: up to 160 / 224 states the one-read kernels leave the
// last two blocks (padding rows only) out of the staging, the operand step and the matrix instructions
int quad_live_blocks(const mbar_ctx* c) { return c->opt_quad_trim ? (int)((c->K + 15) / 16) : 0; }

hipError_t fold_weights(mbar_ctx* w, hipStream_t stream, double alpha, const double*& logden) {
    if (!w->weighted) return hipSuccess;
    hipError_t e = launch_shift_logden(stream, logden, w->cw, alpha, w->N, w->lden_eff);
    logden = w->lden_eff;
    return e;
}

std::vector<double> padded_operand(const double* f, int64_t K, int64_t rows) {
    std::vector<double> an((size_t)rows, -std::numeric_limits<double>::infinity());
    std::copy(f, f + K, an.begin());
    return an;
}

int fetch_red(mbar_ctx* c, size_t total) {
    int rc = allreduce_dev(c, c->red, (int64_t)total, 0);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->hred, c->red, total * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return sync_stream(c);
}

int reserve_gram(mbar_ctx* c, const GramPlan& plan, bool pmode, std::vector<LaunchGeom>* geom) {
    const int64_t ntiles = (c->N + TS - 1) / TS;
    RecordNeed need;
    if (geom) geom->clear();
    for (const auto& it : plan.items) {
        LaunchGeom g;
        if (!it.diag && it.nbj == 16) {  // P mode: rectangle against a 256-state panel, four waves on one shared tile stream
            if (!pmode) return fail(c, MBAR_ERR_STATE, "run_gram: the 256-column rectangles exist on the probability matrix only");
            g = gram_quad_geometry(it.nbi + 16, c->num_cu, ntiles, c->opt_grid);
            if (it.nbi == 8 && c->opt_rect_waves == 8) {  // two waves per SIMD, 16 blocks each (+ their copies of the tile's reciprocals)
                g.waves = 8;
                g.lds_bytes += 2 * 4 * 1024;
            }
        } else if (it.diag && it.nbi > 8) {  // one read of the matrix: the four waves of a workgroup split the panel's blocks
            g = gram_quad_geometry(it.nbi, c->num_cu, ntiles, c->opt_grid);
            g.live_blocks = pmode ? 0 : quad_live_blocks(c);
        } else {
            g = gram_geometry(it.diag ? it.nbi * 16 : (it.nbi + it.nbj) * 16, it.diag, c->num_cu, ntiles, c->opt_grid);
        }
        need.add(g.nwaves, (size_t)it.nblk * 256);
        if (geom) geom->push_back(g);
    }
    return reserve(c, need);
}

// Gram pass with operand exp(anum_k - u_kn - logden_n); anum (device) has Kp entries.
// Results: gram blocks at red + red_off (plan order).  The per-state operand sums are not accumulated on the
// device: rows of p sum to one (sum_k p_nk = 1, resp. sum_k N_k W_nk = 1), so they are column sums of the
// reduced Gram matrix (gram_operand_sums below).
// pmat (or nullptr: the reduced potentials) = a resident probability matrix, `logden` then the reciprocals 1 / s_n with the
// multiplicities' roots already folded in (P mode of the host-driven loop above 256 states: panels and rectangles only)
int run_gram(mbar_ctx* c, const double* anum_dev, const double* logden, size_t red_off, const GramPlan& plan, const double* pmat) {
    const double* mat = pmat ? pmat : c->u;
    std::vector<LaunchGeom> geom;
    int rc = reserve_gram(c, plan, pmat != nullptr, &geom);  // every item's records fit before the first item is launched
    if (rc) return rc;
    if (!pmat) HIPCHK(c, fold_weights(c, c->stream, 0.5, logden));  // sum_n c_n p p^T: each operand carries sqrt(c_n), folded into the exponent
    for (size_t i = 0; i < plan.items.size(); ++i) {
        const auto& it = plan.items[i];
        const LaunchGeom& g = geom[i];
        LoopCtl lo;
        lo.pmode = pmat != nullptr;  // (then: the rows of the probability matrix, `logden` = reciprocals)
        rc = launch_and_reduce(c, g.nwaves, (size_t)it.nblk * 256, c->red + red_off + it.off * 256, [&]() -> int {
            if (!it.diag && it.nbj == 16) {
                HIPCHK(c, launch_gram_rect(c->stream, it.nbi, g, pmat, c->ld, c->N, it.ri, it.rj, logden, c->part));
            } else if (it.diag && it.nbi > 8) {
                HIPCHK(c, launch_gram_quad(c->stream, it.nbi, g, mat + it.ri * c->ld, c->ld, c->N, anum_dev + it.ri, logden, c->part, lo));
            } else if (it.diag) {
                lo.unclamped = c->u_checked && !c->u_posinf;
                HIPCHK(c, launch_gram_diag(c->stream, it.nbi, g, mat, c->ld, c->N, anum_dev + it.ri, logden, it.ri, c->part, nullptr, lo));
            } else {
                HIPCHK(c, launch_gram_off(c->stream, it.nbj, g, mat, c->ld, c->N, anum_dev + it.ri, anum_dev + it.rj, logden, it.ri, it.rj,
                                          c->part, pmat != nullptr));
            }
            return MBAR_OK;
        });
        if (rc) return rc;
    }
    return MBAR_OK;
}

// out_j = sum_k w_k G[k][j]  (w = 1: operand sums of the p-mode Gram; w = N_k: sum_n W_nj of the W-mode Gram)
void gram_operand_sums(const double* G, int64_t K, const double* w, double* out) {
    for (int64_t j = 0; j < K; ++j) out[j] = 0.0;
    for (int64_t k = 0; k < K; ++k) {
        const double wk = w ? w[k] : 1.0;
        if (wk == 0.0) continue;
        for (int64_t j = 0; j < K; ++j) out[j] += wk * G[k * K + j];
    }
}

void gram_row_sums(const double* blocks, int nb, int64_t K, double* psum) {
    std::vector<double> acc((size_t)nb * 16, 0.0);
    int b = 0;
    for (int I = 0; I < nb; ++I)
        for (int J = I; J < nb; ++J, ++b) {
            const double* blk = blocks + (size_t)b * 256;
            for (int r = 0; r < 16; ++r)
                for (int q = (I == J ? r : 0); q < 16; ++q) {
                    const double v = blk[r * 16 + q];
                    acc[(size_t)16 * I + r] += v;
                    if (I != J || q != r) acc[(size_t)16 * J + q] += v;
                }
        }
    for (int64_t k = 0; k < K; ++k) psum[k] = acc[(size_t)k];
}

// Scatter reduced blocks (host copy) into a dense symmetric K x K matrix.
void unpack_gram(const GramPlan& plan, const double* blocks, int64_t K, double* G) {
    for (const auto& it : plan.items) {
        int b = 0;
        for (int I = 0; I < it.nbi; ++I) {
            for (int J = it.diag ? I : 0; J < it.nbj; ++J) {
                const double* blk = blocks + (it.off + b) * 256;
                for (int r = 0; r < 16; ++r)
                    for (int q = 0; q < 16; ++q) {
                        const int64_t gi = it.ri + 16 * I + r, gj = it.rj + 16 * J + q;
                        if (gi < K && gj < K) {
                            const double v = blk[r * 16 + q];
                            if (it.diag && I == J) {
                                if (q >= r) { G[gi * K + gj] = v; G[gj * K + gi] = v; }
                            } else {
                                G[gi * K + gj] = v;
                                G[gj * K + gi] = v;
                            }
                        }
                    }
                ++b;
            }
        }
    }
}

// Row pitch of the aden / psum vectors: the padded state count (padded_K() only produces values
// for which the fused kernel has an instantiation: 16..128 step 16, 192, 256).
int64_t lse_rows(const mbar_ctx* c) { return c->Kp; }

// red / hred, part and scratch for everything one evaluation of nf candidates queues (plan: its Gram plan, or NULL): the sweep and
// the Gram launches leave their records in the same buffers, so all of it is sized before the first of them
static int reserve_eval(mbar_ctx* c, int nf, const GramPlan* plan) {
    const int64_t rows = lse_rows(c);
    LaunchGeom g{};
    int rc = ensure_red(c, (size_t)nf * rows + nf + (plan ? plan->total_blocks * 256 : 0));
    if (!rc) rc = reserve(c, lse_need(c, nf, rows, &g));
    if (!rc && plan) rc = reserve_gram(c, *plan, false);
    return rc;
}

// Core of mbar_eval: f points to nf*K doubles on the host.  Leaves logden in ld0/ld1.
int eval_core(mbar_ctx* c, const double* f, int nf, unsigned flags, double* ld0, double* ld1, double* psum,
              double* sumlogden, double* gram) {
    if (c && c->ext_base) return ext_holds_rows_only(c, "evaluation");
    if (!c->have_Nk) return fail(c, MBAR_ERR_STATE, "mbar_ctx_set_Nk has not been called");
    if (nf < 1 || nf > 2) return fail(c, MBAR_ERR_ARG, "nf must be 1 or 2");
    const bool want_gram = (flags & MBAR_EVAL_GRAM) != 0;
    const bool use_off = (flags & MBAR_EVAL_USE_OFFSET) != 0;
    if (use_off && !c->dn) return fail(c, MBAR_ERR_STATE, "objective offset requested but not set");
    {
        int prc = refresh_poison(c);
        if (prc) return prc;
        if (unusable(c, f, nf)) {
            fill_nan(psum, (size_t)nf * c->K);
            fill_nan(sumlogden, nf);
            if (want_gram) fill_nan(gram, (size_t)c->K * c->K);
            c->error = c->u_poison ? "u_kn contains NaN or -inf: all sums are NaN" : "f_k is not finite: all sums are NaN";
            return MBAR_OK;
        }
    }
    // only the log-denominators are asked for, and slot 0 still holds them for this very f: nothing to do
    const bool only_logden = nf == 1 && ld0 == c->logden[0] && !ld1 && !psum && !sumlogden && !want_gram && !use_off;
    if (only_logden && c->ld0_valid && (int64_t)c->ld0_f.size() == c->K && std::equal(f, f + c->K, c->ld0_f.begin())) return MBAR_OK;
    if (ld0 == c->logden[0] || ld1 == c->logden[0]) c->ld0_valid = false;
    const int64_t rows = lse_rows(c);
    GramPlan plan;
    if (want_gram) plan = plan_for(c);
    const size_t n_ps = (size_t)nf * rows, n_obj = nf;
    const size_t off_gram = n_ps + n_obj, n_gram = plan.total_blocks * 256;
    const size_t total = off_gram + n_gram;
    int rc = reserve_eval(c, nf, want_gram ? &plan : nullptr);
    if (rc) return rc;
    // aden -> device.  The fused kernels evaluate a second candidate from the first one's exponentials through
    // the per-state ratio c_k = exp(a'_k - a_k) (row 1); if the two candidates are so far apart that the ratio
    // could over/underflow against the shared shift, fall back to two single-candidate sweeps.
    std::vector<double> h((size_t)nf * rows);
    for (int i = 0; i < nf; ++i) build_aden(c, f + (size_t)i * c->K, h.data() + (size_t)i * rows, rows);
    bool split = false;
    std::vector<double> ratio;  // c_k of the fused two-candidate sweep; applied to its second psum row below
    if (nf == 2 && (use_fast(c) || split_sweep_ok(c, rows))) {
        double dmax = 0.0;
        for (int64_t k = 0; k < rows; ++k) {
            const double a0 = h[k], a1 = h[rows + k];
            const double d = (std::isinf(a0) && std::isinf(a1)) ? 0.0 : a1 - a0;
            dmax = std::max(dmax, std::fabs(d));
            h[rows + k] = std::exp(d);
        }
        split = !(dmax < 300.0);
        if (!split) ratio.assign(h.begin() + rows, h.begin() + 2 * rows);
    }
    if (split) {
        std::vector<double> ps((size_t)2 * c->K), sl(2);
        int rc2 = eval_core(c, f, 1, flags, ld0, nullptr, ps.data(), &sl[0], gram);
        if (rc2) return rc2;
        rc2 = eval_core(c, f + c->K, 1, flags & ~MBAR_EVAL_GRAM, ld1, nullptr, ps.data() + c->K, &sl[1], nullptr);
        if (rc2) return rc2;
        if (psum) std::copy(ps.begin(), ps.end(), psum);
        if (sumlogden) std::copy(sl.begin(), sl.end(), sumlogden);
        return MBAR_OK;
    }
    // (pinned staging: the copy is stream-ordered before the sweep and the host only touches the buffer again after
    // the sweep's results have been read back, so no synchronisation is needed here)
    std::copy(h.begin(), h.end(), c->hstage.p);
    HIPCHK(c, hipMemcpyAsync(d_aden(c), c->hstage, h.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    // One rank, sums only: the last level of the reduction writes into the pinned host buffer itself (it is mapped into the
    // device's address space) -- one copy kernel less per evaluation; the scipy-driven protocol stages call this thirty times
    // per solve and at the sizes pymbar is mostly used at an evaluation IS its launches.
    const bool direct = c->opt_direct_results && c->nranks <= 1 && !c->comm && !stream_transport(c) && use_fast(c) && !want_gram;
    struct RedSwap {
        mbar_ctx* c; double* saved;
        RedSwap(mbar_ctx* c_, bool on) : c(c_), saved(nullptr) { if (on) { saved = c->red.p; c->red.p = c->hred.p; } }
        ~RedSwap() { if (saved) c->red.p = saved; }
    };
    {
        RedSwap swap(c, direct);
        rc = run_lse(c, nf, rows, ld0, ld1, use_off);
    }
    if (rc) return rc;
    if (want_gram) {
        // p-mode operand: anum = aden of f[0] (Kp entries)
        std::vector<double> an((size_t)c->Kp);
        build_aden(c, f, an.data(), c->Kp);
        std::copy(an.begin(), an.end(), c->hstage + 2 * c->Kp);
        HIPCHK(c, hipMemcpyAsync(d_anum(c), c->hstage + 2 * c->Kp, an.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
        rc = run_gram(c, d_anum(c), ld0, off_gram, plan);
        if (rc) return rc;
    }
    rc = direct ? sync_stream(c) : fetch_red(c, total);
    if (rc) return rc;
    if (!ratio.empty())  // the fused sweep accumulates sum_n e_nk / s'_n for the second candidate: times c_k = its psum
        for (int64_t k = 0; k < rows; ++k) c->hred[(size_t)rows + k] *= ratio[(size_t)k];
    if (psum)
        for (int i = 0; i < nf; ++i)
            for (int64_t k = 0; k < c->K; ++k) psum[(size_t)i * c->K + k] = c->hred[(size_t)i * rows + k];
    if (sumlogden)
        for (int i = 0; i < nf; ++i) sumlogden[i] = c->hred[n_ps + i];
    if (want_gram && gram) {
        std::fill(gram, gram + (size_t)c->K * c->K, 0.0);
        unpack_gram(plan, c->hred + off_gram, c->K, gram);
    }
    if (c->opt_check_finite) {
        for (size_t i = 0; i < n_ps + n_obj; ++i)
            if (!std::isfinite(c->hred[i])) {
                // not fatal for the caller's control flow (the reference also propagates NaN), but flagged
                c->error = "non-finite partial sum in evaluation pass";
                break;
            }
    }
    if (nf == 1 && ld0 == c->logden[0]) {
        c->ld0_f.assign(f, f + c->K);
        c->ld0_valid = true;
    }
    return MBAR_OK;
}

int pass_logden(mbar_ctx* c, const double* f, bool* nan_out) {
    int rc = eval_core(c, f, 1, 0, c->logden[0], nullptr, nullptr, nullptr, nullptr);
    if (rc) return rc;
    *nan_out = unusable(c, f);
    return MBAR_OK;
}

int lognum_sweep(mbar_ctx* c, mbar_ctx* den, std::vector<double>& hm, std::vector<double>& hs) {
    const int64_t nch = lognum_chunks(c->N, c->K);
    int rc = ensure(c, c->lognum_part, (size_t)2 * c->K * nch + 2 * c->K);
    if (rc) return rc;
    double* pmax = c->lognum_part;
    double* psum = pmax + (size_t)c->K * nch;
    double* omax = psum + (size_t)c->K * nch;
    double* osum = omax + c->K;
    HIPCHK(c, hipMemsetAsync(d_anum(c), 0, (size_t)c->Kp * sizeof(double), c->stream));  // anum = 0
    const double* lden = den->logden[0];
    HIPCHK(c, fold_weights(den, c->stream, 1.0, lden));  // log sum_n c_n exp(...) = log sum_n exp(... + ln c_n)
    {
        ScopedTimer t(c, MBAR_TIMER_OTHER);
        HIPCHK(c, launch_lognum(c->stream, c->u, c->ld, c->N, c->K, d_anum(c), lden, pmax, psum, nch));
        HIPCHK(c, launch_lognum_merge(c->stream, pmax, psum, c->K, nch, omax, osum));
    }
    hm.resize(c->K);
    hs.resize(c->K);
    HIPCHK(c, hipMemcpyAsync(hm.data(), omax, c->K * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(hs.data(), osum, c->K * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return sync_stream(c);
}

}  // namespace host
}  // namespace mbar

extern "C" {

int mbar_eval(mbar_ctx* c, const double* f, int nf, unsigned flags, double* psum, double* sumlogden, double* gram) {
    if (!c || !f) return fail(c, MBAR_ERR_ARG, "NULL argument");
    HIPCHK(c, hipSetDevice(c->device));
    return eval_core(c, f, nf, flags, c->logden[0], c->logden[1], psum, sumlogden, gram);
}

int mbar_ctx_set_objective_offset(mbar_ctx* c, const double* f0) {
    if (!c) return fail(c, MBAR_ERR_ARG, "NULL argument");
    HIPCHK(c, hipSetDevice(c->device));
    if (!f0) {
        c->dn.reset();
        return MBAR_OK;
    }
    DevBuf<double> tmp = std::move(c->dn);  // (the context has no offset while the sweep writes the new one)
    int rc = reserve_eval(c, 1, nullptr);  // (before a new vector's zero fill is queued)
    if (!rc) rc = need_zeroed_vec(c, tmp);
    if (rc) return rc;
    rc = eval_core(c, f0, 1, 0, tmp, nullptr, nullptr, nullptr, nullptr);
    c->dn = std::move(tmp);
    return rc;
}

int mbar_logden(mbar_ctx* c, const double* f, double* out_n) {
    if (!c || !f || !out_n) return fail(c, MBAR_ERR_ARG, "NULL argument");
    HIPCHK(c, hipSetDevice(c->device));
    bool nan = false;
    int rc = pass_logden(c, f, &nan);
    if (rc) return rc;
    if (nan) {
        fill_nan(out_n, c->N);
        return MBAR_OK;
    }
    HIPCHK(c, hipMemcpyAsync(out_n, c->logden[0], (size_t)c->N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return sync_stream(c);
}

int mbar_lognum(mbar_ctx* c, const double* f, double* lognum) {
    if (!c || !f || !lognum) return fail(c, MBAR_ERR_ARG, "NULL argument");
    HIPCHK(c, hipSetDevice(c->device));
    bool nan = false;
    int rc = pass_logden(c, f, &nan);
    if (rc) return rc;
    if (nan) {
        fill_nan(lognum, c->K);
        return MBAR_OK;
    }
    std::vector<double> hm, hs;
    rc = lognum_sweep(c, c, hm, hs);
    if (rc) return rc;
    if (c->nranks > 1) {
        std::vector<double> gm = hm;
        for (int64_t k0 = 0; k0 < c->K; k0 += 4 * c->Kp) {
            const int64_t cnt = std::min<int64_t>(4 * c->Kp, c->K - k0);
            rc = allreduce_host(c, gm.data() + k0, cnt, 1);
            if (rc) return rc;
        }
        for (int64_t k = 0; k < c->K; ++k) hs[k] = (hm[k] == gm[k]) ? hs[k] : hs[k] * std::exp(hm[k] - gm[k]);
        for (int64_t k0 = 0; k0 < c->K; k0 += 4 * c->Kp) {
            const int64_t cnt = std::min<int64_t>(4 * c->Kp, c->K - k0);
            rc = allreduce_host(c, hs.data() + k0, cnt, 0);
            if (rc) return rc;
        }
        hm = gm;
    }
    for (int64_t k = 0; k < c->K; ++k) lognum[k] = hm[k] + std::log(hs[k]);
    return MBAR_OK;
}

static int logw_impl(mbar_ctx* c, const double* f, double* out_kn, int64_t ld_out, bool exponentiate) {
    if (!c || !f || !out_kn || ld_out < c->N) return fail(c, MBAR_ERR_ARG, "bad argument");
    HIPCHK(c, hipSetDevice(c->device));
    bool nan = false;
    int rc = pass_logden(c, f, &nan);
    if (rc) return rc;
    if (nan) {
        for (int64_t k = 0; k < c->K; ++k) fill_nan(out_kn + k * ld_out, c->N);
        return MBAR_OK;
    }
    // stream the result through a device staging buffer in row blocks to bound extra memory
    const int64_t rows_per = std::max<int64_t>(1, std::min<int64_t>(c->K, (int64_t)((256ull << 20) / ((size_t)c->ld * 8))));
    DevBuf<double> stage;
    HIPCHK(c, stage.grow((size_t)rows_per * c->ld));
    HIPCHK(c, hipMemcpyAsync(d_f(c), f, c->K * sizeof(double), hipMemcpyHostToDevice, c->stream));
    for (int64_t k0 = 0; k0 < c->K; k0 += rows_per) {
        const int64_t nr = std::min(rows_per, c->K - k0);
        {
            ScopedTimer t(c, MBAR_TIMER_OTHER);
            hipError_t e = launch_logw(c->stream, c->u + k0 * c->ld, c->ld, c->N, nr, d_f(c) + k0, c->logden[0], stage, c->ld, exponentiate);
            if (e != hipSuccess) return fail(c, MBAR_ERR_HIP, hipGetErrorString(e));
        }
        hipError_t e = hipMemcpy2DAsync(out_kn + k0 * ld_out, (size_t)ld_out * sizeof(double), stage,
                                        (size_t)c->ld * sizeof(double), (size_t)c->N * sizeof(double), (size_t)nr,
                                        hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return fail(c, MBAR_ERR_HIP, hipGetErrorString(e));
    }
    flush_timers(c);
    return MBAR_OK;
}
int mbar_logw(mbar_ctx* c, const double* f, double* out_kn, int64_t ld_out) { return logw_impl(c, f, out_kn, ld_out, false); }
int mbar_w(mbar_ctx* c, const double* f, double* out_kn, int64_t ld_out) { return logw_impl(c, f, out_kn, ld_out, true); }

int mbar_gram_w(mbar_ctx* c, const double* f, double* gramW, double* wsum) {
    if (!c || !f) return fail(c, MBAR_ERR_ARG, "NULL argument");
    HIPCHK(c, hipSetDevice(c->device));
    bool nan = false;
    int rc = pass_logden(c, f, &nan);
    if (rc) return rc;
    if (nan) {
        fill_nan(gramW, (size_t)c->K * c->K);
        fill_nan(wsum, c->K);
        return MBAR_OK;
    }
    GramPlan plan = plan_for(c);
    const size_t n_gram = plan.total_blocks * 256, total = n_gram;
    rc = ensure_red(c, total);
    if (rc) return rc;
    const std::vector<double> an = padded_operand(f, c->K, c->Kp);
    HIPCHK(c, hipMemcpyAsync(d_anum(c), an.data(), an.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    rc = run_gram(c, d_anum(c), c->logden[0], 0, plan);
    if (rc) return rc;
    rc = fetch_red(c, total);
    if (rc) return rc;
    std::vector<double> Gtmp(gramW ? 0 : (size_t)c->K * c->K);
    double* G = gramW ? gramW : Gtmp.data();
    std::fill(G, G + (size_t)c->K * c->K, 0.0);
    unpack_gram(plan, c->hred, c->K, G);
    if (wsum) gram_operand_sums(G, c->K, c->Nk.data(), wsum);  // sum_n W_nj = sum_k N_k (W^T W)_kj
    return MBAR_OK;
}

}  // extern "C"
