// gfx950 (CDNA4 / MI355X) kernels of mbar_batch: many small MBAR problems (K <= 64 states each) solved side by side.  One of the
// translation units of libmbar_hip.so: launchers declared in mbar_batch.h, C ABI in mbar_batch.cpp, design and numbers in
// DESIGN.md ("Many small MBAR problems").
//
// Every problem's columns are cut into chunks of MBAR_BATCH_CHUNK samples; one workgroup of 256 threads handles one chunk, one
// sample per thread, with the sample's K reduced potentials in registers.  Chunks are launched in four width classes (8, 16, 32,
// 64 states) so that a problem of 5 states does not carry 64 registers of padding; a problem always lands in the same class.
//   k_batch_eval   at each f the problem's state requests (one or two): the log-denominator of every sample, then per state the
//                  chunk maximum of -logden_n - u_kn and the sum of exp(. - maximum) (log space: no term is lost to underflow
//                  that is not below 2^-1074 of the chunk's largest), and at one request the K x K Gram partial of
//                  p_nk = N_k W_nk (or of W itself for the covariance).  The per-state sums go through an LDS transposition,
//                  16 states at a time; the Gram matrix is VALU outer products of 64-sample tiles staged in LDS, each thread
//                  owning a 1x1, 2x2 or 4x4 block.
//   k_batch_step   one workgroup per problem: merges the chunk partials in chunk order, advances the problem's adaptive loop
//                  (batch_advance, mbar_batch.h) and, when it asks for one, factors the gauge-fixed Newton system in LDS
//                  (LDL^T, one barrier pair per pivot).
//   k_batch_draw   bootstrap draw counts of many replica slots in one launch (the counter-based stream of mbar_common.h).
//   k_batch_ext_*  the extension rows of the problems (new states and observables of the expectation family, MBARBatch): per row
//                  the chunk maximum and scaled sum in log space (k_batch_ext_sums, merged by k_batch_ext_sums_merge), and the
//                  augmented Gram matrix Q^T Q of up to 128 columns, Q = [W | the rows' weight columns] (k_batch_ext_gram: 32-sample
//                  tiles in LDS, each thread a block of up to 8x8, one record per run of MBAR_BATCH_EXT_RUN chunks, merged in run
//                  order by k_batch_ext_gram_merge).
// Replica slots (bootstrap replicates, BatchData in mbar_batch.h) share their base problem's block and run the weighted
// instantiation of k_batch_eval: sample n counts c_n >= 0 times.  Its log-denominator is unchanged; the chunk maximum of a state
// is taken over the samples with c_n > 0 and its sum is sum_n c_n exp(. - maximum); the Gram operands are scaled by sqrt(c_n) when
// the tile is staged, so that sum_n c_n q q^T stays bit-symmetric.  k_batch_step does not know about multiplicities.
// No floating-point atomics but one: the draw counts, sums of 1.0 (exact, whatever the order).  Every other sum has a fixed order
// that depends on the problem alone, so two identical calls return identical bits and a problem's (or a slot's) answer does not
// depend on the other problems of the batch.
#include "mbar_device.h"
#include "mbar_batch.h"

namespace mbar {

namespace {

constexpr int TP = MBAR_BATCH_CHUNK + 1;  // pitch of the per-state transposition tile (16 states x 256 samples)

template <int KB, bool WT = false>
__global__ void __launch_bounds__(BATCH_WG) k_batch_eval(BatchData d, const int* __restrict__ list,
                                                         const mbar_batch_state* __restrict__ states) {
    constexpr int GS = KB < 16 ? KB : 16;   // states per transposition group
    constexpr int BS = KB >= 64 ? 4 : (KB >= 32 ? 2 : 1);  // Gram block per thread
    constexpr int NBD = KB / BS;            // Gram blocks per dimension (NBD^2 <= 256)
    constexpr int GP = KB + 1;              // pitch of the Gram operand tile (64 samples x KB states)
    __shared__ double buf[64 * 65];         // (the two tiles share one buffer)
    static_assert(64 * 65 >= 16 * TP && 64 * 65 >= 64 * GP, "tile sizes");
    __shared__ double sa[2][KB];
    __shared__ double sg[KB];
    __shared__ int info[4];
    __shared__ double sc[WT ? MBAR_BATCH_CHUNK : 1];  // (weighted form: the chunk's multiplicities)
    const int tid = threadIdx.x;
    const int c = list[blockIdx.x];
    const int p = d.cprob[c];
    const mbar_batch_state* st = states + p;
    if (tid == 0) {
        info[0] = (int)st->nreq;
        info[1] = (int)st->gram_req;
        info[2] = (int)st->K;
        info[3] = (int)st->gram_w;
    }
    __syncthreads();
    const int nreq = info[0] > 2 ? 2 : info[0], greq = info[1], K = info[2], gw = info[3];
    if (nreq <= 0) return;  // (the problem has ended: the whole workgroup leaves)
    if (tid < KB) {
        const bool on = tid < K && st->Nk[tid] > 0;
        const double lnN = on ? log(st->Nk[tid]) : 0.0;
        for (int r = 0; r < nreq; ++r) sa[r][tid] = on ? st->req[r][tid] + lnN : -INFINITY;
        if (greq >= 0 && greq < nreq)
            sg[tid] = tid >= K ? -INFINITY : (gw ? st->req[greq][tid] : (on ? st->req[greq][tid] + lnN : -INFINITY));
    }
    const int64_t Np = d.N[p];
    const int64_t n0 = d.cn0[c];
    const int ncols = (int)(Np - n0 < MBAR_BATCH_CHUNK ? Np - n0 : MBAR_BATCH_CHUNK);
    const bool valid = tid < ncols;
    const double* __restrict__ up = d.u + d.uoff[p] + n0 + tid;
    double u[KB];
#pragma unroll
    for (int k = 0; k < KB; ++k) u[k] = (valid && k < K) ? up[(int64_t)k * Np] : INFINITY;
    double* __restrict__ rec = d.part + d.coff[c];
    double cq = 1.0;  // sqrt(c_n)
    if constexpr (WT) {
        const double cn = valid ? d.cw[d.cwoff[p] + n0 + tid] : 0.0;
        sc[tid] = cn;
        cq = sqrt(cn);
    }
    __syncthreads();
    for (int r = 0; r < nreq; ++r) {
        // log-denominator of this sample: log sum_k N_k exp(f_k - u_kn)
        double m = -INFINITY;
#pragma unroll
        for (int k = 0; k < KB; ++k) m = fmax(m, sa[r][k] - u[k]);
        double ld = INFINITY;  // (a padding column, or one with no finite sampled entry: every term below is exp(-inf) = 0)
        if (m != -INFINITY) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < KB; ++k) s += exp((sa[r][k] - u[k]) - m);
            ld = m + log(s);
        }
        // per state: maximum over the chunk of v_k = -logden - u_k and the sum of exp(v_k - maximum)
#pragma unroll
        for (int g0 = 0; g0 < KB; g0 += GS) {
            if (g0 >= K) break;
            __syncthreads();
#pragma unroll
            for (int j = 0; j < GS; ++j) {
                if constexpr (WT) buf[j * TP + tid] = cq > 0.0 ? -ld - u[g0 + j] : -INFINITY;  // (a sample not drawn: no term)
                else buf[j * TP + tid] = -ld - u[g0 + j];
            }
            __syncthreads();
            const int kk = tid >> 4, q = tid & 15;
            double mx = -INFINITY;
            if (kk < GS)
#pragma unroll 4
                for (int i = 0; i < MBAR_BATCH_CHUNK / 16; ++i) mx = fmax(mx, buf[kk * TP + q + 16 * i]);
            mx = row16_max(mx);
            double sm = 0.0;
            if (kk < GS && mx != -INFINITY)
#pragma unroll 4
                for (int i = 0; i < MBAR_BATCH_CHUNK / 16; ++i) {
                    if constexpr (WT) sm += sc[q + 16 * i] * exp(buf[kk * TP + q + 16 * i] - mx);
                    else sm += exp(buf[kk * TP + q + 16 * i] - mx);
                }
            sm = row16_sum(sm);
            if (q == 0 && kk < GS && g0 + kk < K) {
                rec[r * K + g0 + kk] = mx;
                rec[2 * K + r * K + g0 + kk] = sm;
            }
        }
        if (r != greq) continue;
        // Gram partial: sum over the chunk's samples of q q^T, q_k = exp(sg_k - u_k - logden), 64 samples at a time
        const int wv = tid >> 6, lane = tid & 63;
        const int bi = tid / NBD, bj = tid % NBD;
        double acc[BS][BS];
#pragma unroll
        for (int a = 0; a < BS; ++a)
#pragma unroll
            for (int b = 0; b < BS; ++b) acc[a][b] = 0.0;
        for (int w = 0; w < BATCH_WG / 64; ++w) {
            if (w * 64 >= ncols) break;
            __syncthreads();
            if (wv == w)
#pragma unroll
                for (int k = 0; k < KB; ++k) {
                    if constexpr (WT) buf[lane * GP + k] = cq > 0.0 ? cq * exp((sg[k] - u[k]) - ld) : 0.0;
                    else buf[lane * GP + k] = exp((sg[k] - u[k]) - ld);
                }
            __syncthreads();
            if (tid < NBD * NBD) {
                const int cols = ncols - w * 64 < 64 ? ncols - w * 64 : 64;
                for (int j = 0; j < cols; ++j) {
                    double x[BS], y[BS];
#pragma unroll
                    for (int a = 0; a < BS; ++a) {
                        x[a] = buf[j * GP + bi * BS + a];
                        y[a] = buf[j * GP + bj * BS + a];
                    }
#pragma unroll
                    for (int a = 0; a < BS; ++a)
#pragma unroll
                        for (int b = 0; b < BS; ++b) acc[a][b] += x[a] * y[b];
                }
            }
        }
        if (tid < NBD * NBD)
#pragma unroll
            for (int a = 0; a < BS; ++a)
#pragma unroll
                for (int b = 0; b < BS; ++b) {
                    const int i = bi * BS + a, j = bj * BS + b;
                    if (i < K && j < K) rec[4 * K + i * K + j] = acc[a][b];
                }
    }
}

__global__ void __launch_bounds__(BATCH_WG) k_batch_step(BatchData d, mbar_batch_state* __restrict__ states, int* __restrict__ active,
                                                         double* __restrict__ out_gram, double* __restrict__ out_wsum,
                                                         const int64_t* __restrict__ goff, const int64_t* __restrict__ woff) {
    constexpr int MK = MBAR_BATCH_MAX_K;
    __shared__ mbar_batch_state st;
    __shared__ double G[MK * MK];
    __shared__ double ln[2 * MK];
    __shared__ double b[MK];
    __shared__ int idx[MK];
    __shared__ int sh_m;
    __shared__ double sh_thr, sh_gbar;
    const int tid = threadIdx.x;
    const int p = blockIdx.x;
    {
        static_assert(sizeof(mbar_batch_state) % 8 == 0, "state copied as 8-byte words");
        constexpr int W = (int)(sizeof(mbar_batch_state) / 8);
        const uint64_t* src = reinterpret_cast<const uint64_t*>(states + p);
        uint64_t* dst = reinterpret_cast<uint64_t*>(&st);
        for (int i = tid; i < W; i += BATCH_WG) dst[i] = src[i];
    }
    __syncthreads();
    const int nreq = (int)(st.nreq > 2 ? 2 : st.nreq);
    if (nreq <= 0) {
        if (tid == 0) active[p] = 0;
        return;
    }
    const int K = (int)st.K, greq = (int)st.gram_req;
    const int64_t cb = d.cbeg[p], ce = d.cbeg[p + 1];
    // merge in chunk order: per state the maximum of the chunk maxima, then the rescaled sums
    for (int r = 0; r < nreq; ++r)
        if (tid < K) {
            double M = -INFINITY;
            for (int64_t c = cb; c < ce; ++c) M = fmax(M, d.part[d.coff[c] + r * K + tid]);
            double S = 0.0;
            if (M != -INFINITY)
                for (int64_t c = cb; c < ce; ++c) {
                    const double* rec = d.part + d.coff[c];
                    const double s = rec[2 * K + r * K + tid];
                    if (s != 0.0) S += s * exp(rec[r * K + tid] - M);
                }
            ln[r * K + tid] = M == -INFINITY ? -INFINITY : M + log(S);
        }
    if (greq >= 0 && greq < nreq)
        for (int e = tid; e < K * K; e += BATCH_WG) {
            double s = 0.0;
            for (int64_t c = cb; c < ce; ++c) s += d.part[d.coff[c] + 4 * K + e];
            G[(e / K) * MK + e % K] = s;
        }
    __syncthreads();
    if (st.phase == BATCH_PH_FINAL) {
        // the covariance inputs at the final f: W^T W and sum_n W_nk = exp(f_k + lognum_k)
        for (int e = tid; e < K * K; e += BATCH_WG) out_gram[goff[p] + e] = G[(e / K) * MK + e % K];
        if (tid < K) out_wsum[woff[p] + tid] = exp(st.req[0][tid] + ln[tid]);
        if (tid == 0) {
            states[p].nreq = 0;
            states[p].phase = BATCH_PH_IDLE;
            active[p] = 0;
        }
        return;
    }
    if (tid == 0) batch_advance(st, ln);
    __syncthreads();
    if (st.phase == BATCH_PH_NEWTON) {
        if (tid == 0) {
            const int s0 = batch_first_sampled(st);
            int m = 0;
            for (int k = 0; k < K; ++k)
                if (st.Nk[k] > 0 && k != s0) idx[m++] = k;
            sh_m = m;
            sh_thr = batch_pivot_threshold(st, m);
            sh_gbar = batch_gradient_mean(st);
        }
        __syncthreads();
        const int m = sh_m;
        const double thr = sh_thr;
        // H = diag(psum) - G of the live states, compacted in place through registers; b = the gradient psum - N_k less its mean
        double v[MK * MK / BATCH_WG];
#pragma unroll
        for (int j = 0; j < MK * MK / BATCH_WG; ++j) {
            const int e = tid + j * BATCH_WG;
            if (e < m * m) {
                const int i = e / m, jj = e % m;
                v[j] = (i == jj ? st.psum[idx[i]] : 0.0) - G[idx[i] * MK + idx[jj]];
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < MK * MK / BATCH_WG; ++j) {
            const int e = tid + j * BATCH_WG;
            if (e < m * m) G[(e / m) * MK + e % m] = v[j];
        }
        if (tid < m) b[tid] = (st.psum[idx[tid]] - st.Nk[idx[tid]]) - sh_gbar;
        __syncthreads();
        // LDL^T (the serial batch_ldlt_solve, one pivot per barrier pair) with the forward substitution folded in
        bool ok = true;
        for (int j = 0; j < m; ++j) {
            const double dj = G[j * MK + j];
            if (!(dj > thr) || !isfinite(dj)) {
                ok = false;
                break;
            }
            const int n = m - j - 1;
            for (int e = tid; e < n * n; e += BATCH_WG) {
                const int i = j + 1 + e / n, k = j + 1 + e % n;
                if (k <= i) G[i * MK + k] = G[i * MK + k] - (G[i * MK + j] / dj) * G[k * MK + j];
            }
            if (tid > j && tid < m) b[tid] = b[tid] - (G[tid * MK + j] / dj) * b[j];
            __syncthreads();
            if (tid > j && tid < m) G[tid * MK + j] = G[tid * MK + j] / dj;
            __syncthreads();
        }
        if (ok) {
            if (tid < m) b[tid] = b[tid] / G[tid * MK + tid];
            __syncthreads();
            for (int j = m - 1; j > 0; --j) {
                if (tid < j) b[tid] = b[tid] - G[j * MK + tid] * b[j];
                __syncthreads();
            }
        }
        if (tid == 0) {
            st.newton_bad = ok ? 0 : 1;
            for (int k = 0; k < K; ++k) st.x[k] = 0.0;
            if (ok)
                for (int i = 0; i < m; ++i) st.x[idx[i]] = b[i];
            batch_advance(st, nullptr);
        }
    }
    __syncthreads();
    {
        constexpr int W = (int)(sizeof(mbar_batch_state) / 8);
        const uint64_t* src = reinterpret_cast<const uint64_t*>(&st);
        uint64_t* dst = reinterpret_cast<uint64_t*>(states + p);
        for (int i = tid; i < W; i += BATCH_WG) dst[i] = src[i];
    }
    if (tid == 0) active[p] = st.nreq > 0 ? 1 : 0;
}

// Draw counts of replica slots.  Chunk c of slot s = cprob[c]: thread t holds position j = cn0[c] + t of the slot's N[s] draws, in
// the run [cum[k], cum[k + 1]) of its state k, and adds 1.0 to the count of the sample it draws (exact in any order).
__global__ void __launch_bounds__(BATCH_WG) k_batch_draw(BatchData d, int64_t chunk0, const int64_t* __restrict__ base,
                                                         const int64_t* __restrict__ Kp, const int64_t* __restrict__ cum,
                                                         const uint64_t* __restrict__ seed, const int64_t* __restrict__ replicate,
                                                         double* __restrict__ cw) {
    const int64_t c = chunk0 + blockIdx.x;
    const int s = d.cprob[c];
    const int64_t j = d.cn0[c] + threadIdx.x;
    if (j >= d.N[s]) return;
    const int64_t b = base[s];
    const int64_t* __restrict__ cm = cum + b * (MBAR_BATCH_MAX_K + 1);
    int64_t lo = 0, hi = Kp[b];  // the state k with cum[k] <= j < cum[k + 1] (empty states have empty runs)
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (cm[mid] <= j) lo = mid; else hi = mid;
    }
    const int64_t start = cm[lo], nk = cm[lo + 1] - start;
    const int64_t pos = start + bootstrap_draw(seed[s], (uint64_t)replicate[s], (uint64_t)j, (uint64_t)nk);
    if (pos >= 0 && pos < d.N[s]) atomicAdd(cw + d.cwoff[s] + pos, 1.0);
}

// ---- extension rows (mbar_batch_set_ext): the expectation family of a batch -------------------------------------------------
// The augmented matrix of a problem has up to MBAR_BATCH_MAX_AUG = 128 columns, twice what a thread of k_batch_eval can keep in
// registers, so these kernels hold nothing per sample but its log-denominator and read the rows where they use them.

// sa[k] = f_k + log N_k of the sampled states, -inf otherwise (thread k < K; the caller synchronises)
__device__ __forceinline__ void ext_load_sa(const BatchExt& x, int p, int K, double* sa) {
    const int tid = threadIdx.x;
    if (tid < K) {
        const double nk = x.Nk[(int64_t)p * MBAR_BATCH_MAX_K + tid];
        sa[tid] = nk > 0 ? x.f[(int64_t)p * MBAR_BATCH_MAX_K + tid] + log(nk) : -INFINITY;
    }
}

// log sum_k N_k exp(f_k - u_kn) of the sample at `up` (its column, rows Np apart): the expression and the order of k_batch_eval
__device__ __forceinline__ double ext_logden(const double* __restrict__ up, int64_t Np, int K, const double* sa) {
    double m = -INFINITY;
    for (int k = 0; k < K; ++k) m = fmax(m, sa[k] - up[(int64_t)k * Np]);
    if (m == -INFINITY) return INFINITY;  // (no finite sampled entry: every term of this sample is exp(-inf) = 0)
    double s = 0.0;
    for (int k = 0; k < K; ++k) s += exp((sa[k] - up[(int64_t)k * Np]) - m);
    return m + log(s);
}

// Per extension row the chunk maximum of v_r = -logden_n - e_rn and the sum of exp(v_r - maximum): k_batch_eval's per-state sums,
// 16 rows at a time through the same transposition tile.  One workgroup per chunk of the problems.
__global__ void __launch_bounds__(BATCH_WG) k_batch_ext_sums(BatchData d, BatchExt x) {
    __shared__ double buf[16 * TP];
    __shared__ double sa[MBAR_BATCH_MAX_K];
    const int tid = threadIdx.x;
    const int c = blockIdx.x;
    const int p = d.cprob[c];
    const int R = (int)x.R[p], K = (int)x.K[p];
    if (!x.mask[p] || R == 0) return;  // (the whole workgroup)
    ext_load_sa(x, p, K, sa);
    __syncthreads();
    const int64_t Np = d.N[p];
    const int64_t n0 = d.cn0[c];
    const int ncols = (int)(Np - n0 < MBAR_BATCH_CHUNK ? Np - n0 : MBAR_BATCH_CHUNK);
    const bool valid = tid < ncols;
    const double ld = valid ? ext_logden(d.u + d.uoff[p] + n0 + tid, Np, K, sa) : INFINITY;
    const double* __restrict__ ep = x.e + x.eoff[p] + n0 + tid;
    double* __restrict__ rec = x.lpart + x.lcoff[c];
    const int kk = tid >> 4, q = tid & 15;
    for (int g0 = 0; g0 < R; g0 += 16) {
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < 16; ++j) buf[j * TP + tid] = (valid && g0 + j < R) ? -ld - ep[(int64_t)(g0 + j) * Np] : -INFINITY;
        __syncthreads();
        double mx = -INFINITY;
#pragma unroll 4
        for (int i = 0; i < MBAR_BATCH_CHUNK / 16; ++i) mx = fmax(mx, buf[kk * TP + q + 16 * i]);
        mx = row16_max(mx);
        double sm = 0.0;
        if (mx != -INFINITY)
#pragma unroll 4
            for (int i = 0; i < MBAR_BATCH_CHUNK / 16; ++i) sm += exp(buf[kk * TP + q + 16 * i] - mx);
        sm = row16_sum(sm);
        if (q == 0 && g0 + kk < R) {
            rec[g0 + kk] = mx;
            rec[R + g0 + kk] = sm;
        }
    }
}

// One workgroup per problem: the chunk records of its rows merged in chunk order, as k_batch_step merges the states'
__global__ void __launch_bounds__(BATCH_WG) k_batch_ext_sums_merge(BatchData d, BatchExt x, double* __restrict__ out) {
    const int p = blockIdx.x;
    const int R = (int)x.R[p];
    if (!x.mask[p]) return;
    const int64_t cb = d.cbeg[p], ce = d.cbeg[p + 1];
    for (int r = threadIdx.x; r < R; r += BATCH_WG) {
        double M = -INFINITY;
        for (int64_t c = cb; c < ce; ++c) M = fmax(M, x.lpart[x.lcoff[c] + r]);
        double S = 0.0;
        if (M != -INFINITY)
            for (int64_t c = cb; c < ce; ++c) {
                const double* rec = x.lpart + x.lcoff[c];
                const double s = rec[R + r];
                if (s != 0.0) S += s * exp(rec[r] - M);
            }
        out[x.roff[p] + r] = M == -INFINITY ? -INFINITY : M + log(S);
    }
}

// Q^T Q and the column sums of Q over one run of MBAR_BATCH_EXT_RUN consecutive chunks of a problem, Q = [W | exp(f_ext_r - e_rn -
// logden_n)], A = K + R <= AB columns.  Tiles of 32 samples x A columns are staged in LDS (33 KB at AB = 128); the 256 threads form
// a 16 x 16 grid and thread (bi, bj) owns the (AB/16)^2 entries (bi + 16 a, bj + 16 b), so that a half-wave reads 16 consecutive
// doubles of a tile row (no bank conflict) and 2 broadcast ones.  Entries (i, j) and (j, i) add the same products x_i x_j in the
// same sample order: G is bit-symmetric.  The accumulators live in registers across the run, whose record is written once.
template <int AB>
__global__ void __launch_bounds__(BATCH_WG) k_batch_ext_gram(BatchData d, BatchExt x, const int* __restrict__ wprob,
                                                             const int* __restrict__ wrun, const int64_t* __restrict__ wgoff,
                                                             double* __restrict__ gpart) {
    constexpr int BS = AB / 16;  // entries per thread and dimension
    constexpr int TS = 32;       // samples per tile
    constexpr int GP = AB + 1;   // pitch of a tile row
    __shared__ double buf[TS * GP];
    __shared__ double sa[MBAR_BATCH_MAX_K];
    __shared__ double sg[AB];
    __shared__ double sld[MBAR_BATCH_CHUNK];
    const int tid = threadIdx.x;
    const int p = wprob[blockIdx.x];
    const int K = (int)x.K[p], R = (int)x.R[p], A = K + R;
    ext_load_sa(x, p, K, sa);
    if (tid < AB) sg[tid] = tid < K ? x.f[(int64_t)p * MBAR_BATCH_MAX_K + tid] : (tid < A ? x.fext[x.roff[p] + tid - K] : 0.0);
    const int64_t Np = d.N[p];
    const double* __restrict__ ub = d.u + d.uoff[p];
    const double* __restrict__ eb = R > 0 ? x.e + x.eoff[p] : ub;
    const int64_t c0 = d.cbeg[p] + (int64_t)wrun[blockIdx.x] * MBAR_BATCH_EXT_RUN;
    const int64_t c1 = c0 + MBAR_BATCH_EXT_RUN < d.cbeg[p + 1] ? c0 + MBAR_BATCH_EXT_RUN : d.cbeg[p + 1];
    const int bi = tid >> 4, bj = tid & 15;
    const int sj = tid & (TS - 1), sc0 = tid / TS;  // staging: sample sj of the tile, columns sc0, sc0 + 8, ...
    double acc[BS][BS];
#pragma unroll
    for (int a = 0; a < BS; ++a)
#pragma unroll
        for (int b = 0; b < BS; ++b) acc[a][b] = 0.0;
    double cs = 0.0;  // column sum of column tid
    __syncthreads();
    for (int64_t c = c0; c < c1; ++c) {
        const int64_t n0 = d.cn0[c];
        const int ncols = (int)(Np - n0 < MBAR_BATCH_CHUNK ? Np - n0 : MBAR_BATCH_CHUNK);
        // (the last reads of sld for the chunk before lie ahead of the barrier that precedes its last tile's products)
        sld[tid] = tid < ncols ? ext_logden(ub + n0 + tid, Np, K, sa) : INFINITY;
        for (int t0 = 0; t0 < ncols; t0 += TS) {
            __syncthreads();
            const bool in = t0 + sj < ncols;
            const double ldn = sld[t0 + sj];
            const int64_t n = n0 + t0 + sj;
            for (int col = sc0; col < AB; col += BATCH_WG / TS) {
                double v = 0.0;
                if (in && col < A) {
                    const double e = col < K ? ub[(int64_t)col * Np + n] : eb[(int64_t)(col - K) * Np + n];
                    v = exp((sg[col] - e) - ldn);
                }
                buf[sj * GP + col] = v;
            }
            __syncthreads();
            const int cols = ncols - t0 < TS ? ncols - t0 : TS;
            for (int j = 0; j < cols; ++j) {
                double xr[BS], yr[BS];
#pragma unroll
                for (int a = 0; a < BS; ++a) {
                    xr[a] = buf[j * GP + bi + 16 * a];
                    yr[a] = buf[j * GP + bj + 16 * a];
                }
#pragma unroll
                for (int a = 0; a < BS; ++a)
#pragma unroll
                    for (int b = 0; b < BS; ++b) acc[a][b] += xr[a] * yr[b];
            }
            if (tid < A)
                for (int j = 0; j < cols; ++j) cs += buf[j * GP + tid];
        }
    }
    double* __restrict__ rec = gpart + wgoff[blockIdx.x];
#pragma unroll
    for (int a = 0; a < BS; ++a)
#pragma unroll
        for (int b = 0; b < BS; ++b) {
            const int i = bi + 16 * a, j = bj + 16 * b;
            if (i < A && j < A) rec[i * A + j] = acc[a][b];
        }
    if (tid < A) rec[A * A + tid] = cs;
}

// One workgroup per problem of the group: its runs' records summed in run order
__global__ void __launch_bounds__(BATCH_WG) k_batch_ext_gram_merge(BatchExt x, const int* __restrict__ gprob,
                                                                   const int64_t* __restrict__ gbase, const int* __restrict__ nrun,
                                                                   const double* __restrict__ gpart, double* __restrict__ ogram,
                                                                   double* __restrict__ owsum, const int64_t* __restrict__ ogoff,
                                                                   const int64_t* __restrict__ owoff) {
    const int p = gprob[blockIdx.x];
    const int A = (int)(x.K[p] + x.R[p]);
    const int sz = A * A + A, nr = nrun[blockIdx.x];
    const double* __restrict__ rec = gpart + gbase[blockIdx.x];
    for (int e = threadIdx.x; e < sz; e += BATCH_WG) {
        double s = 0.0;
        for (int r = 0; r < nr; ++r) s += rec[(int64_t)r * sz + e];
        if (e < A * A) ogram[ogoff[p] + e] = s;
        else owsum[owoff[p] + e - A * A] = s;
    }
}

template <bool WT>
hipError_t launch_eval(hipStream_t st, int kb, const BatchData& d, const int* list, int64_t n, const mbar_batch_state* states) {
    switch (kb) {
    case 8: hipLaunchKernelGGL((k_batch_eval<8, WT>), dim3((unsigned)n), dim3(BATCH_WG), 0, st, d, list, states); break;
    case 16: hipLaunchKernelGGL((k_batch_eval<16, WT>), dim3((unsigned)n), dim3(BATCH_WG), 0, st, d, list, states); break;
    case 32: hipLaunchKernelGGL((k_batch_eval<32, WT>), dim3((unsigned)n), dim3(BATCH_WG), 0, st, d, list, states); break;
    case 64: hipLaunchKernelGGL((k_batch_eval<64, WT>), dim3((unsigned)n), dim3(BATCH_WG), 0, st, d, list, states); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace

hipError_t launch_batch_eval(hipStream_t st, int kb, const BatchData& d, const int* list, int64_t n, const mbar_batch_state* states) {
    if (n == 0) return hipSuccess;
    if (d.cw && !d.cwoff) return hipErrorInvalidValue;
    return d.cw ? launch_eval<true>(st, kb, d, list, n, states) : launch_eval<false>(st, kb, d, list, n, states);
}

hipError_t launch_batch_draw(hipStream_t st, const BatchData& d, int64_t chunk0, int64_t nchunk, const int64_t* base,
                             const int64_t* Kp, const int64_t* cum, const uint64_t* seed, const int64_t* replicate, double* cw) {
    if (nchunk == 0) return hipSuccess;
    hipLaunchKernelGGL(k_batch_draw, dim3((unsigned)nchunk), dim3(BATCH_WG), 0, st, d, chunk0, base, Kp, cum, seed, replicate, cw);
    return hipGetLastError();
}

hipError_t launch_batch_step(hipStream_t st, const BatchData& d, mbar_batch_state* states, int* active, double* out_gram,
                             double* out_wsum, const int64_t* goff, const int64_t* woff) {
    if (d.P == 0) return hipSuccess;
    hipLaunchKernelGGL(k_batch_step, dim3((unsigned)d.P), dim3(BATCH_WG), 0, st, d, states, active, out_gram, out_wsum, goff, woff);
    return hipGetLastError();
}

hipError_t launch_batch_ext_lognum(hipStream_t st, const BatchData& d, const BatchExt& x, double* lognum_ext) {
    if (d.P == 0 || d.nchunks == 0) return hipSuccess;
    hipLaunchKernelGGL(k_batch_ext_sums, dim3((unsigned)d.nchunks), dim3(BATCH_WG), 0, st, d, x);
    hipLaunchKernelGGL(k_batch_ext_sums_merge, dim3((unsigned)d.P), dim3(BATCH_WG), 0, st, d, x, lognum_ext);
    return hipGetLastError();
}

hipError_t launch_batch_ext_gram(hipStream_t st, int ab, const BatchData& d, const BatchExt& x, int64_t n, const int* wprob,
                                 const int* wrun, const int64_t* wgoff, double* gpart) {
    if (n == 0) return hipSuccess;
    switch (ab) {
    case 16: hipLaunchKernelGGL(k_batch_ext_gram<16>, dim3((unsigned)n), dim3(BATCH_WG), 0, st, d, x, wprob, wrun, wgoff, gpart); break;
    case 32: hipLaunchKernelGGL(k_batch_ext_gram<32>, dim3((unsigned)n), dim3(BATCH_WG), 0, st, d, x, wprob, wrun, wgoff, gpart); break;
    case 64: hipLaunchKernelGGL(k_batch_ext_gram<64>, dim3((unsigned)n), dim3(BATCH_WG), 0, st, d, x, wprob, wrun, wgoff, gpart); break;
    case 128: hipLaunchKernelGGL(k_batch_ext_gram<128>, dim3((unsigned)n), dim3(BATCH_WG), 0, st, d, x, wprob, wrun, wgoff, gpart); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_batch_ext_gram_merge(hipStream_t st, const BatchExt& x, int64_t n, const int* gprob, const int64_t* gbase,
                                       const int* nrun, const double* gpart, double* ogram, double* owsum, const int64_t* ogoff,
                                       const int64_t* owoff) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_batch_ext_gram_merge, dim3((unsigned)n), dim3(BATCH_WG), 0, st, x, gprob, gbase, nrun, gpart, ogram, owsum,
                       ogoff, owoff);
    return hipGetLastError();
}

}  // namespace mbar
