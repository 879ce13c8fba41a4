// ---- reweighting scans over a linear family of unsampled states, and the histogram surfaces along a scan (mbar_k_scan.hip;
// panels, tables, bin groups and C ABI in mbar_scan.cpp) ------------------------------------------------------------------------
#pragma once
#include "mbar_common.h"

namespace mbar {

constexpr int SCAN_MAX_B = MBAR_SCAN_MAX_B;  // basis vectors
constexpr int SCAN_MAX_Q = MBAR_SCAN_MAX_Q;  // observables
constexpr int SCAN_VCHUNK = 2048;            // samples of one wave of pass A
constexpr int SCAN_CHUNK = 8192;             // samples of one workgroup of pass B: the cut of N depends on N alone
// blocks of 16 members per wave of pass B for J = 1 + Q operand columns per member, and per-member sums of its vec record
constexpr int scan_mb(int J) { return J == 1 ? 4 : J == 2 ? 2 : 1; }
constexpr int scan_nv(int J) { return 1 + J + J * (J + 1) / 2; }
constexpr int SCANBIN_NV = 2;  // per (member, bin) sums of a binned pass-B record: wsum | diag
struct ScanData {
    int64_t N, ldv;
    int B, Q;
    const double* basis;   // [B][ldv]
    const double* t;       // [Q][ldv] shifted observables (> 0)
    const double* logden;  // [N]
    const double* cw;      // [N] multiplicities (NULL: 1)
};
// The samples sorted by bin (perm: sorted position -> sample, ascending n inside a bin) and cut into chunks that never straddle a
// bin: chunk c of a table belongs to bin chunk_bin[c] and is that bin's chunk number c - bin_chunk0[bin], positions bin_start[bin]
// + chunk number x chunk length onward.  With one bin holding every sample the cut is the cut of the scan passes.
struct ScanBinTable {
    int64_t nchunks = 0;
    const int32_t* chunk_bin = nullptr;   // [nchunks]
    const int64_t* bin_chunk0 = nullptr;  // [nbins + 1]
};
struct ScanBins {
    int64_t nbins;
    const int32_t* perm;       // [bin_start[nbins]]
    const int64_t* bin_start;  // [nbins + 1]
};
// The cut of the samples a launch sums over, the compile-time policy of the kernels: the bins [b0(), b1()) and their chunks
// [c0(), c1()) of at most len positions (chunk c0() writes record 0), the positions [p0, p1) of chunk c and its bin, the sample at
// position p.  The whole cut also carries what only it has, the reference member of pass B.
struct ScanWhole {  // every sample in its own order, as one bin: chunk c is [c len, min(N, (c + 1) len))
    static constexpr bool binned = false;
    int64_t ref = 0;
    MBAR_HD int64_t nbins() const { return 1; }
    MBAR_HD int64_t b0() const { return 0; }
    MBAR_HD int64_t b1() const { return 1; }
    MBAR_HD int64_t c0() const { return 0; }
    MBAR_HD int64_t c1(int64_t N, int64_t len) const { return (N + len - 1) / len; }
    MBAR_HD void bin_chunks(int64_t, int64_t N, int64_t len, int64_t& ca, int64_t& cb) const { ca = 0, cb = c1(N, len); }
    MBAR_HD void range(int64_t c, int64_t N, int64_t len, int64_t& bin, int64_t& p0, int64_t& p1) const {
        bin = 0;
        p0 = c * len;
        p1 = p0 + len < N ? p0 + len : N;
    }
    MBAR_HD int64_t sample(int64_t p) const { return p; }
};
struct ScanBinned {  // the sorted positions of the bins [b0_, b1_), whose chunks in table t are [c0_, c1_)
    static constexpr bool binned = true;
    ScanBins sb;
    ScanBinTable t;
    int64_t b0_, b1_, c0_, c1_;
    MBAR_HD int64_t nbins() const { return sb.nbins; }
    MBAR_HD int64_t b0() const { return b0_; }
    MBAR_HD int64_t b1() const { return b1_; }
    MBAR_HD int64_t c0() const { return c0_; }
    MBAR_HD int64_t c1(int64_t, int64_t) const { return c1_; }
    MBAR_HD void bin_chunks(int64_t bin, int64_t, int64_t, int64_t& ca, int64_t& cb) const { ca = t.bin_chunk0[bin], cb = t.bin_chunk0[bin + 1]; }
    MBAR_HD void range(int64_t c, int64_t, int64_t len, int64_t& bin, int64_t& p0, int64_t& p1) const {
        bin = t.chunk_bin[c];
        const int64_t end = sb.bin_start[bin + 1];
        p0 = sb.bin_start[bin] + (c - t.bin_chunk0[bin]) * len;
        p1 = p0 + len < end ? p0 + len : end;
    }
    MBAR_HD int64_t sample(int64_t p) const { return sb.perm[p]; }
};
// The kind of the terms of a member, the second compile-time policy of the scan kernels (and, as FamilyTerms, the wave-uniform
// argument of the family fill): u_l(n) = offset[l] + sum_b term_b, b ascending, a linear term fma(coeff, basis, u), a harmonic one
//   dl = basis - center;  P > 0: m = rint(dl rP), dl = fma(-P, m, dl);  u = fma(coeff, dl dl, u)
// (family_term in mbar_scan_device.h: every operation rounded once).  ScanLinear is the family of mbar_ctx_set_scan alone: its
// instantiations carry no trace of the other kind.
constexpr int SCAN_MAX_H = MBAR_SCAN_MAX_H;  // harmonic terms
struct FamilyTerms {
    uint32_t mask = 0;           // bit b: term b is harmonic
    double period[SCAN_MAX_B];   // P_b of a harmonic term (0: not periodic)
    double rperiod[SCAN_MAX_B];  // 1.0 / P_b, rounded once on the host (0 where P_b = 0)
};
struct ScanLinear {
    static constexpr bool harmonic = false;
    static constexpr int mb(int J) { return scan_mb(J); }
    MBAR_HD ScanLinear from(int64_t) const { return *this; }
};
struct ScanHarmonic {
    static constexpr bool harmonic = true;
    // narrower panels of pass B than the linear family's: with its members' centres next to the coefficients the widest
    // instantiations (8 blocks of states) would not fit the register file at 4 (J = 1) or 2 (J = 2) blocks of members per wave
    static constexpr int mb(int J) { return J == 1 ? 2 : 1; }
    FamilyTerms terms;
    const double* center;  // [L][SCAN_MAX_H] on the device: the centres of the harmonic terms in ascending b, zeros behind them
    MBAR_HD ScanHarmonic from(int64_t l0) const {  // the family as the members [l0, L) see it
        ScanHarmonic h = *this;
        h.center += l0 * SCAN_MAX_H;
        return h;
    }
};
// Where the observables t_j of a member come from, the third compile-time policy of the two sweeps.  ScanStored: t_jn is read from
// ScanData::t, the same for every member -- what every instantiation had before the policy existed, and they carry no trace of the
// other kind.  ScanEnergy: the member's own reduced potential, formed from the value the chain produced for x_ln,
//   t_0 = 1,  t_1 = u_l(n) - center_u[l],  t_2 = t_1 t_1        (J = 1 + ScanData::Q = 2 or 3; ScanData::t is not read)
// every operation rounded once.  Pass B then keeps two rows of products with the reference member r where the stored kind keeps
// one, because t_r1 is the reference member's own: vec = wsum | refblock[i < 2][J] | within[i <= j],
// refblock[l][i][j] = sum_n c_n (b_rn t_ri)(b_ln t_lj).  Whole cut only.
struct ScanStored {
    static constexpr bool energy = false;
    static constexpr int ref_rows = 1;
    static constexpr int nv(int J) { return scan_nv(J); }
    template <class Fam>
    static constexpr int mb(int J) { return Fam::mb(J); }
    MBAR_HD ScanStored from(int64_t) const { return *this; }
};
struct ScanEnergy {
    static constexpr bool energy = true;
    static constexpr int ref_rows = 2;
    static constexpr int nv(int J) { return 1 + 2 * J + J * (J + 1) / 2; }
    // the stored kind's widths at J = 2, 3: the per-member sums are wider (J more) and the centre rides along, and still no
    // instantiation uses scratch (the compiler's report is in DESIGN.md section 21)
    template <class Fam>
    static constexpr int mb(int J) { return Fam::harmonic || J > 2 ? 1 : 2; }
    const double* center_u;  // [L] on the device
    MBAR_HD ScanEnergy from(int64_t l0) const { return ScanEnergy{center_u + l0}; }
};
// ScanMoments: the stored observables AND the features the chain is made of, for the derivatives of f and of the averages along
// a scan (mbar_scan_moments).  Pass A on the whole cut only, in a sweep of its own (k_scan_moments): term b
// hands out phi = basis[b][n] when linear and dl_b, dl_b^2 (the wrapped displacement family_term formed) when harmonic, and member l
// accumulates, with d_i = phi_i - center_phi[l][i] and e = c_n exp(x_ln - M_l),
//   S0 = sum e | S_q = sum e t_qn | A_i = sum e d_i | B_ij = sum e d_i d_j (i <= j) | C_qi = sum e t_qn d_i
// every difference and product rounded once, every accumulation one fma.  The kernel keeps the features in SLOTS that are static in
// the term: the squares of the harmonic terms, in ascending b, in slots [0, hb), the term's own value (basis or dl) in slot hb + b;
// a bucket (hb, bb) serves the families with at most hb harmonic terms among at most bb, slots nobody fills carry exact zeros.  The
// host maps slots to the features of the C ABI (ascending b: a linear term's basis, a harmonic term's dl then dl^2).
struct ScanMoments {
    int hb = 0, bb = 0;                  // the bucket: one of (0, 2), (0, 8) under ScanLinear, (1, 3), (4, 8) under ScanHarmonic
    const double* center_phi = nullptr;  // [L][hb + bb] on the device, by slot
    MBAR_HD int slots() const { return hb + bb; }
    // doubles of a (chunk, member) record, of a member's merged sums: S0 | S[Q] | A[slots] | B[slots (slots + 1) / 2] | C[Q][slots]
    MBAR_HD int record(int Q) const { return 1 + Q + slots() + slots() * (slots() + 1) / 2 + Q * slots(); }
    MBAR_HD ScanMoments from(int64_t l0) const { return ScanMoments{hb, bb, center_phi + l0 * slots()}; }
};
// (scan_moments_bucket in mbar_scan_moments.h: the smallest bucket that serves a family)
// the sums of the members [0, L) of coeff / offset / mom.center_phi about the maxima M[L] (of launch_scan_vec, sum = false, ScanStored):
// rec[chunk][record][L], and their merge in chunk order: lognum[L] and out[L][record] = the sums over S0 (out[l][0] = 1)
template <class Fam>
hipError_t launch_scan_moments(hipStream_t s, const ScanData& d, const Fam& fam, const ScanMoments& mom, int64_t L, const double* coeff,
                               const double* offset, const double* M, double* rec);
hipError_t launch_scan_moments_merge(hipStream_t s, const ScanData& d, const ScanMoments& mom, int64_t L, const double* rec, const double* M,
                                     double* lognum, double* out);
// Cut = ScanWhole or ScanBinned (Q = 0), Fam = ScanLinear or ScanHarmonic, Obs = ScanStored or ScanEnergy (whole cut, Q = 1 or 2) in
// the two sweeps; the merges know neither family kind (the cross merge is told the panel width and the record's Obs).
// pass A over the members [0, L) of coeff / offset: per-chunk records of the maxima (sum = false: rec[chunk][L]) or of the J scaled
// sums (rec[chunk][L][J]), and their merge in chunk order into M[bin][L] (bin-major, of this member panel), or into
// lognum[l][bin] (row pitch nbins) and, on the whole cut, mean[L][J]
// (the maxima do not depend on the observables: sum = false is the ScanStored launch under either Obs)
template <class Cut, class Fam, class Obs>
hipError_t launch_scan_vec(hipStream_t s, const ScanData& d, const Cut& cut, const Fam& fam, const Obs& obs, bool sum, int64_t L,
                           const double* coeff, const double* offset, const double* M, double* rec);
template <class Cut>
hipError_t launch_scan_vec_merge(hipStream_t s, const ScanData& d, const Cut& cut, bool sum, int64_t L, const double* rec, double* M,
                                 double* lognum, double* mean);
// pass B for the panel of members [p0, p0 + 64 mb) of L, mb = Obs::mb<Fam>(J): part[chunk - c0][scan_record_doubles(nb, J, nv, mb)],
// then cross[k][l][bin][j] (K x L x nbins x J) and vec[l][bin][nv].  Whole cut: nv = Obs::nv(J), vec = wsum | refcol[J] (ScanEnergy:
// refblock[2][J]) | within[i <= j], fnorm = f_scan[L]; binned cut: J = 1, nv = SCANBIN_NV, vec = wsum | diag, fnorm = f_bins[L][nbins] (+inf: an empty bin of that
// member, exact zeros).  nb = scan_nb_for(K) blocks of 16 states, or 0: no cross block.
int scan_nb_for(int64_t K);
int64_t scan_record_doubles(int nb, int J, int nv, int mb);
template <class Cut, class Fam, class Obs>
hipError_t launch_scan_cross(hipStream_t s, const ScanData& d, const Cut& cut, const Fam& fam, const Obs& obs, int nb, const double* u,
                             int64_t ld, int64_t K, const double* f, int64_t L, int64_t p0, const double* coeff, const double* offset,
                             const double* fnorm, double* part);
template <class Cut, class Obs>
hipError_t launch_scan_cross_merge(hipStream_t s, const ScanData& d, const Cut& cut, int nb, int mb, int64_t K, int64_t L, int64_t p0,
                                   const double* part, double* cross, double* vec);
// The member-member Gram block (mbar_scan_pair_gram), whole cut, stored observables, either family:
//   pair[r][l][i][j] = sum_n c_n (b_{rows[r]} n t_in)(b_ln t_jn)
// One launch per (row panel, member panel): the row panel is the rm <= scan_pair_rows(nb, J) reference members rows[0 .. rm) (on the
// device, indices into the call's L members) as 16 nb rows (member, i) of the LDS tile, nb = 2 or 8 (scan_pair_nb_for(reference
// members left, J)); the member panel is [p0, p0 + 64 mb), mb = Fam::mb(J).  part[chunk][scan_pair_record_doubles(nb, J, mb)], then
// the merge in chunk order into pair (at the row panel's first reference member: rows of L J J doubles).
constexpr int scan_pair_rows(int nb, int J) { return 16 * nb / J; }
int scan_pair_nb_for(int64_t R, int J);
int64_t scan_pair_record_doubles(int nb, int J, int mb);
template <class Fam>
hipError_t launch_scan_pair(hipStream_t s, const ScanData& d, const Fam& fam, int nb, int64_t L, int64_t p0, const int64_t* rows, int rm,
                            const double* coeff, const double* offset, const double* fnorm, double* part);
hipError_t launch_scan_pair_merge(hipStream_t s, const ScanData& d, int nb, int mb, int64_t L, int64_t p0, int rm, const double* part,
                                  double* pair);
// Many observables along a scan (mbar_scan_obs_sums), whole cut, either family: pass B with the rows of the LDS
// tile being nq <= 16 nb stored observables a[nq][d.ldv] (nb = scan_nb_for(nq)) instead of sampled states.  mode 0: s1 = sum c b a;
// mode 1: s1 and t1 = sum c b b a (two operand columns per member); mode 2: t2 = sum c b b a a (the fill stage squares the tile).
// One launch per (member panel [p0, p0 + 64 mb), observable panel, mode), mb = Fam::mb(scan_obs_columns(mode));
// part[chunk][scan_obs_record_doubles(nb, J, mb)], then the merge in chunk order into out0 / out1 (column 0 / 1; L x Q row-major, at
// observable qb) and, where asked for (the first observable panel), wsum into vec0[L] and w2sum into vec1[L].
int scan_obs_columns(int mode);
int64_t scan_obs_record_doubles(int nb, int J, int mb);
template <class Fam>
hipError_t launch_scan_obs(hipStream_t s, const ScanData& d, const Fam& fam, int nb, int mode, const double* a, int64_t nq, int64_t L,
                           int64_t p0, const double* coeff, const double* offset, const double* fnorm, double* part);
hipError_t launch_scan_obs_merge(hipStream_t s, const ScanData& d, int nb, int mode, int mb, int64_t L, int64_t Q, int64_t p0, int64_t qb,
                                 int64_t nq, const double* part, double* out0, double* out1, double* vec0, double* vec1);
// Kernel-density surfaces along a scan (mbar_scan_kde_sums), whole cut, either family:
// launch_scan_obs at mode 0 with the tile COMPUTED, k(q_i, x_n) = exp(-r^2 / 2h^2) of the queries [qb, qb + nq) of q[d][ldq] against
// the points x[d][d.ldv] (nq <= 16 nb, nb = scan_nb_for(nq), d = 1 or 2).  One launch per (member panel [p0, p0 + 64 mb), query
// panel), mb = Fam::mb(1); part[chunk][scan_kde_record_doubles(nb, mb)], then the merge in chunk order into logsum[L][M] (log of the
// sum; NaN where the sum is not >= 2^-900) and, where asked for, wsum[L].  launch_scan_kde_exact: out[i] = the log of the sum of pair
// (member pairs[2 i], query pairs[2 i + 1]) in plain log space, one workgroup each.
constexpr int SCANKDE_MAX_D = 2;
struct ScanKde {
    int d;
    const double* x;  // [d][ScanData::ldv] the points of the samples
    const double* q;  // [d][ldq] the queries
    int64_t ldq, M;
    double coef;   // -S log2(e) / 2h^2: the exp2s argument of a pair is r^2 coef
    double inv_h;  // 1 / h
    double period[SCANKDE_MAX_D], rperiod[SCANKDE_MAX_D];  // P_k (0: not periodic) and 1.0 / P_k, rounded once on the host
};
ScanKde scan_kde_make(int d, const double* x, const double* q, int64_t ldq, int64_t M, double h, const double* period);
int64_t scan_kde_record_doubles(int nb, int mb);
template <class Fam>
hipError_t launch_scan_kde(hipStream_t s, const ScanData& d, const Fam& fam, const ScanKde& kd, int nb, int64_t qb, int64_t nq, int64_t L,
                           int64_t p0, const double* coeff, const double* offset, const double* fnorm, double* part);
hipError_t launch_scan_kde_merge(hipStream_t s, const ScanData& d, const ScanKde& kd, int nb, int mb, int64_t L, int64_t p0, int64_t qb,
                                 int64_t nq, const double* part, double* logsum, double* wsum);
template <class Fam>
hipError_t launch_scan_kde_exact(hipStream_t s, const ScanData& d, const Fam& fam, const ScanKde& kd, int64_t npairs, const int64_t* pairs,
                                 const double* coeff, const double* offset, const double* fnorm, double* out);

// ---- rows of the resident matrix from a family of states (mbar_k_family.hip; C ABI: mbar_ctx_fill_family_rows and ----------
// ---- mbar_ctx_fill_linear_rows in mbar_rows.cpp) -----------------------------------------------------------------------------
constexpr int FILL_THREADS = 256;      // a lane owns two adjacent columns: 512 columns per workgroup and pass
constexpr int FILL_ROWS = 128;         // rows a lane writes from one read of its basis values (grid.y = row groups)
constexpr int FILL_MAX_BLOCKS = 2048;  // grid.x; the column pairs go round it
// rows[r][n] = offset[r] + sum_b term_b for r < nrows, n < N: the chain of family_term and scan_x, b ascending.  rows (pitch ld) and
// basis (pitch ldb) 16-byte aligned with even pitches; coeff[nrows][B], center[nrows][B], offset[nrows] on the device.
// terms.mask == 0, every term linear, rows[r][n] = fma(coeff[r][B-1], basis[B-1][n], ... fma(coeff[r][0], basis[0][n], offset[r])):
// the ScanLinear instantiation, which never reads center (NULL will do); otherwise the FamilyTerms one
hipError_t launch_fill_rows(hipStream_t s, double* rows, int64_t ld, int64_t N, int64_t nrows, int B, const double* basis, int64_t ldb,
                            const double* coeff, const double* center, const double* offset, const FamilyTerms& terms);

}  // namespace mbar
