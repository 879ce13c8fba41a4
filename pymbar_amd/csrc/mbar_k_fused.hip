// gfx950 (CDNA4 / MI355X) kernels of the MBAR solver hot path -- the fused sweep of the device-resident adaptive loop: k_fused.
// One of the translation units of libmbar_hip.so (compiled in parallel by pymbar_amd/_build.py): the shared device helpers and
// the data-layout notes are in mbar_sweep_device.h, the host-side interface of the launchers in mbar_internal.h.
#include "mbar_sweep_device.h"

namespace mbar {

// ---------------------------------------------------------------------------------------------
// Fused sweep of the device-resident loop in P mode: ONE pass over the resident probability matrix per iteration.
// For the two candidates (multipliers cmul[0] = f_sci, cmul[1] = f_nr relative to the anchor) it does what k_psweep does --
// normalisers 1 / s_n into the slot vectors, per-state sums -- and, from the SAME tile in LDS, accumulates the Gram
// matrix of the Newton-Raphson candidate on the matrix cores, G'_nr = sum_n (P_n / s_n^nr)(P_n / s_n^nr)^T.  If the loop
// then accepts f_nr (it nearly always does: mbar_solvers.py:607) the next iteration's Hessian is already there and the
// separate Gram sweep is skipped; otherwise that sweep runs (k_select decides, CTL_NEEDGRAM).
// One wave per SIMD owns the register file (288 accumulator registers), so nothing hides behind another wave: every
// instruction that is not under an executing matrix instruction costs its issue slot, fp64 VALU work shares the matrix pipe,
// and an LDS-DMA instruction stalls the wave for tens of cycles.  The tile loop is therefore laid out by hand
// (profiles/r2_fused_sweep_anatomy.txt):
//   * the normalisers are 4x4x4 matrix instructions on a second read of the tile (32 x 16 cycles instead of 64 FMAs,
//     128 DPP moves, 32 adds and eight reciprocals), computed one tile AHEAD between the Gram blocks of groups 2 and 3;
//   * Gram operands are fetched one group ahead, the multiplier operands in two batches, all behind issued matrix work;
//   * the tile after next is requested piece by piece between the Gram blocks of group 3 (the buffer is free then);
//   * the 8 NB per-state accumulations stay where they are written (the compiler would sink them to the loop end and keep
//     all four groups' operands alive), and a tile's body is ONE basic block (the register allocator handles the pinned
//     accumulators only then);
//   * beyond the matrix instructions the vector pipe gets arithmetic only (profiles/fused_tile_loop_vector_census_ab.txt; full
//     panel, unit weights: 80 instructions per tile -- 32 products, 32 + 2 + 2 multiply-adds, 3 additions, a maximum, a reciprocal
//     seed, one compare and two selects for a ragged tile, four broadcasts).  The loop runs TWO tiles per trip, buffer 0 then
//     buffer 1, so that an LDS address is a loop-invariant lane register + an immediate; its bookkeeping (tiles left, samples
//     of the next tile, source and slot addresses) is 32-bit scalar arithmetic; the reciprocals go out through a scalar base +
//     a fixed lane offset under a lane mask written out by hand; and the first candidate's broadcast rides in the DPP operand
//     of its multiply-add (UNIT).
// wsq: sqrt of the per-sample multiplicities (= cw itself for plain 0 / 1 weights).
// UNIT: every sample counts once (a context without sample weights: cw is a vector of ones) -- the tile carries no weights' piece,
// no group reads or multiplies by w / sw (x * 1.0 is exact: the results are the general kernel's to the bit), and the 4 NB
// multiplier operands of the 4x4x4 steps, which never change during a launch, sit in registers instead of being read from LDS
// every tile (full panel: 52 -> 32 LDS read instructions, 17 -> 16 LDS-DMA pieces and 40 -> 32 multiplications per tile, 440
// of 512 registers).  A sample beyond N, which the general kernel drops through its multiplicity of zero, gets the reciprocal
// zero there (store_rinv: one select per tile) -- its column of P is NOT zero when k_build_sweep built the matrix.  Option
// "fused_general" runs the general kernel instead.
// ---------------------------------------------------------------------------------------------
// (Measured dead end, twice: the diagonal 16 x 16 blocks of the full panel as three v_mfma_f64_4x4x4_4b_f64 each -- 48 matrix-pipe
// cycles instead of 64, half of the 16x16x4 block lies below the diagonal.  Round 2, with DPP-rotated copies of the scaled operand:
// 1 % SLOWER (profiles/r2_fused_sweep_anatomy.txt, section 5).  Round 4, with NO vector instruction for it -- the per-sample scale
// on the A side only, G' = sum_n (P_n w_n / s_n^2) P_n^T, every B operand the raw tile entry, the rotated ones read from LDS through a
// rotated lane map -- parity-green and within +-1 % of the 16x16x4 blocks in three alternations on one box
// (profiles/r4_ab_fused_diag_subblocks_from_lds.txt): a 4x4x4 instruction costs the wave more than its 16 pipe cycles.)
// Schedule of the 2 NB 4x4x4 steps a group carries (k_fused): how many have been issued once row I of the group's Gram blocks
// is out.  Narrow panels: two per row, the rest after the last-but-one row.  NB >= 4: the first NB (one operand batch) two per
// row, the second batch spread over the rows that remain before the last.
template <int NB>
__host__ __device__ constexpr int fused_steps_done(int I) {
    if (I < 0) return 0;
    if (I >= NB - 2) return 2 * NB;
    if (NB < 4) return 2 * (I + 1) < 2 * NB ? 2 * (I + 1) : 2 * NB;
    const int r1 = (NB + 1) / 2 - 1;  // row that completes the first batch
    if (I <= r1) return 2 * (I + 1) < NB ? 2 * (I + 1) : NB;
    const int rows = NB - 2 - r1;     // rows r1 + 1 .. NB - 2 share the second batch
    return NB + (NB * (I - r1) + rows - 1) / rows;
}
template <int NB, bool WIDE, bool UNIT>
__global__ void __launch_bounds__(256, 1)
k_fused(const double* __restrict__ P, int64_t ld, int64_t N, int64_t ntiles, const double* __restrict__ cmul,
        const double* __restrict__ cw, const double* __restrict__ wsq, double* __restrict__ rinv0,
        double* __restrict__ rinv1, double* __restrict__ gram_part, double* __restrict__ psum_part,
        const int* __restrict__ ctl, int64_t slot_stride) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (ctl) {
        if (ctl[CTL_DONE] != 0 || ctl[CTL_LIGHT] != 0) return;  // (CTL_LIGHT: the last iteration needs no Gram matrix, see k_psweep)
        const int s = ctl[CTL_SLOT];
        rinv1 = rinv0 + (int64_t)((s + 2) % 3) * slot_stride;
        rinv0 = rinv0 + (int64_t)((s + 1) % 3) * slot_stride;
    }
    constexpr int ROWS = NB * 16;
    constexpr int NDMA = ROWS / 8 + (UNIT ? 0 : 1);         // tile rows + one piece for the two weight vectors
    constexpr int U_BYTES = ROWS * TS * 8;
    constexpr int TILE_BYTES = U_BYTES + (UNIT ? 0 : 1024);  // (the weights' piece is a full-wave LDS-DMA too: no exec-masked branch)
    constexpr int NBLK = NB * (NB + 1) / 2;
    constexpr bool PINNED = NBLK > GRAM_AGPR_BLOCKS;
    // Full panel: the per-state sums of the SECOND candidate are not accumulated here -- the rows of p sum to one, so they are
    // sum_j c_j G'_kj of the Gram matrix this sweep accumulates for that very candidate, and k_select takes them from the
    // reduced blocks (FUSED_PSUM1_FROM_GRAM_NB): 8 NB fp64 instructions less per tile on a pipe the matrix instructions share.
    constexpr bool ACC1 = NB < FUSED_PSUM1_FROM_GRAM_NB;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nwv = blockDim.x >> 6;
    const int ks = lane & 15, ns = lane >> 4;
    char* buf = smem + wave * (2 * TILE_BYTES);
    const int64_t gw = (int64_t)blockIdx.x * nwv + wave;
    const int64_t W = (int64_t)gridDim.x * nwv;
    RowIdentity rows{0};
    StageOffsetsT<WIDE> so = make_stage_offsets<WIDE>(ld, lane);

    double acc[2][NB];
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int I = 0; I < NB; ++I) acc[f][I] = 0.0;
    {   // rows whose multipliers are zero for both candidates (states without samples, padding: their rows of P are zero too)
        double cany[NB];
#pragma unroll
        for (int I = 0; I < NB; ++I) cany[I] = fabs(cmul[16 * I + ks]) + fabs(cmul[ROWS + 16 * I + ks]);
        if constexpr (NB <= 2) rows.live = live_piece_mask<NB>(cany, 0.0);  // (narrow panels only: see k_gram)
    }
    // The normalisers s_n = sum_k P_kn c_k of both candidates come from the matrix pipe as well: v_mfma_f64_4x4x4_4b
    // contracts over lane bits 4-5 (measured lane map, profiles/r2_mfma4x4_probe.txt: A lane = i + 4 b + 16 k, B lane =
    // j + 4 b + 16 k, D lane = j + 4 b + 16 i), so with the tile read a SECOND time as A(sample = lane & 15, state = 4 step +
    // (lane >> 4)) and the multipliers as B(candidate = lane & 3, same state) 32 instructions of 16 cycles leave
    // s[sample (lane >> 4) + 4 ((lane >> 2) & 3)][candidate lane & 3] in one register -- in place of 64 FMAs, 128 DPP moves,
    // 32 adds and eight reciprocals.  The multiplier operand is a 4 KB table behind the wave buffers (UNIT: NSTEP registers, made
    // opaque so that the compiler cannot load them again inside the loop).
    constexpr int NSTEP = ROWS / 4;
    double cb[UNIT ? NSTEP : 1];
    if constexpr (UNIT) {
#pragma unroll
        for (int st = 0; st < NSTEP; ++st) {
            // (lanes of candidates 2 and 3 load candidate (lane & 1)'s entry and drop it: no exec-masked branch per load)
            const double cv = cmul[(lane & 1) * ROWS + 4 * st + (lane >> 4)];
            cb[st] = (lane & 3) < 2 ? cv : 0.0;
            asm volatile("" : "+v"(cb[st]));
        }
    } else {
        double* ctab = reinterpret_cast<double*>(smem + nwv * (2 * TILE_BYTES));
        for (int e = threadIdx.x; e < NSTEP * 16; e += blockDim.x) ctab[e] = (e & 3) < 2 ? cmul[(e & 3) * ROWS + (e >> 2)] : 0.0;
        __syncthreads();
    }
    // LDS read addresses: the lane's part, with the wave's buffers folded in, is formed ONCE (and made opaque, so that the compiler
    // keeps the registers instead of forming the sums again); which of the two buffers, the block row and the step are compile-time
    // constants in the tile loop (two tiles per trip: buffer 0, then buffer 1) and ride in the instructions' offset fields.
    const uint32_t bufo = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)buf;
    uint32_t apos[4];  // second-layout read: row 4 step + k holds sample n at position (n + (row & 14)) & 15
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        apos[q] = bufo + ns * (TS * 8) + (((lane & 15) + (ns & 2) + 4 * q) & 15) * 8;
        asm volatile("" : "+v"(apos[q]));
    }
    v4d G[NBLK];
#pragma unroll
    for (int b = 0; b < NBLK; ++b) G[b] = v4d{0.0, 0.0, 0.0, 0.0};

    uint32_t pos[GROUPS];
#pragma unroll
    for (int g = 0; g < GROUPS; ++g) {
        pos[g] = bufo + ks * (TS * 8) + ((4 * g + ns + (ks & 14)) & 15) * 8;
        asm volatile("" : "+v"(pos[g]));
    }
    [[maybe_unused]] uint32_t wpos = bufo + U_BYTES + ns * 8;  // (general form: the sample's multiplicity behind the tile)
    if constexpr (!UNIT) asm volatile("" : "+v"(wpos));
    const int sq = ns + 4 * ((lane >> 2) & 3);  // the lane's sample and candidate in the layout the 4x4x4 blocks leave
    const int fq = lane & 3;
    // The two slot vectors as ONE wave-uniform base (the lower of the two) + a lane offset that never changes: the lane's sample
    // in the tile, and for the lanes of the candidate whose vector is the upper one the distance between the two.  (Not WIDE:
    // 32 bits -- the launcher takes the WIDE form when 16 slot_stride + 128 does not fit.)  Lanes of the candidates 2 and 3
    // hold no normaliser: their sample index is 16, beyond every tile's count, so that ONE 32-bit compare per tile decides
    // both what is stored and (UNIT) which reciprocals are zeroed.
    const bool up1 = reinterpret_cast<uintptr_t>(rinv1) > reinterpret_cast<uintptr_t>(rinv0);
    char* const rlo = reinterpret_cast<char*>(up1 ? rinv0 : rinv1);
    const uint64_t rgap = up1 ? reinterpret_cast<uintptr_t>(rinv1) - reinterpret_cast<uintptr_t>(rinv0)
                              : reinterpret_cast<uintptr_t>(rinv0) - reinterpret_cast<uintptr_t>(rinv1);
    typename StageOffsetsT<WIDE>::off_t roff = (typename StageOffsetsT<WIDE>::off_t)(((fq == 1) == up1 ? rgap : 0) + sq * 8);
    const int sqs = fq < 2 ? sq : TS;
    const int nlast = (int)(N - (ntiles - 1) * TS);  // samples of the matrix's last tile: 1 .. 16

    // multiplicities and their roots behind the tile: even 128-byte rows of the piece take cw, odd rows wsq (rows 2-7 repeat them)
    const char* wsrc = reinterpret_cast<const char*>(((lane >> 3) & 1) ? wsq : cw) + (lane & 7) * 16;
    auto stage_w = [&](int64_t tile, char* dst) {
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(wsrc + tile * (TS * 8)),
                                         (__attribute__((address_space(3))) void*)(dst + U_BYTES), 16, 0, 0);
    };
    auto stage = [&](int64_t tile, char* dst) {
        stage_tile<ROWS, true, 0, 1>(P, ld, tile * TS, dst, lane, so, rows);
        if constexpr (!UNIT) stage_w(tile, dst);
    };
    // operands of group g in the Gram layout (state 16 I + ks, sample 4 g + ns) + the sample's multiplicity and its root
    // (tb: byte offset of the tile's buffer in the wave's pair, 0 or TILE_BYTES)
    auto lds_at = [](uint32_t a) { return *(lds_cdouble*)(uintptr_t)a; };
    auto read_group = [&](int tb, int g, double (&x)[NB], double& wg, double& swg) {
        if constexpr (!UNIT) {
            wg = lds_at(wpos + (tb + 4 * g * 8));
            swg = lds_at(wpos + (tb + TS * 8 + 4 * g * 8));
        }
#pragma unroll
        for (int I = 0; I < NB; ++I) x[I] = lds_at(pos[g] + (tb + I * (16 * TS * 8)));
    };
    uint32_t cop_off = (uint32_t)(nwv * (2 * TILE_BYTES) + (lane >> 4) * 32 + (lane & 3) * 8);
    auto read_step = [&](int tb, int st, double& a, double& b) {
        a = lds_at(apos[st & 3] + (tb + st * (4 * TS * 8)));
        if constexpr (UNIT) b = cb[st];
        else b = *reinterpret_cast<const double*>(smem + cop_off + st * 128);
    };
    // (first: the accumulator starts from the inline constant 0 -- a register zeroed by a VALU move right in front of an asm
    // matrix instruction, where the hazard recogniser cannot see it, gave wrong sums)
    auto mfma4 = [&](double& d, double a, double b, bool first) {
        if constexpr (PINNED) {
            if (first)
                asm volatile("v_mfma_f64_4x4x4_4b_f64 %0, %1, %2, 0" : "=v"(d) : "v"(a), "v"(b));
            else
                asm volatile("v_mfma_f64_4x4x4_4b_f64 %0, %1, %2, %0" : "+v"(d) : "v"(a), "v"(b));
        } else {
            d = __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, first ? 0.0 : d, 0, 0, 0);
        }
    };
    // nv: the tile's samples that exist, wave-uniform -- 16, the matrix's last tile nlast, a tile past the end 0
    auto store_rinv = [&](int64_t tile, int nv, double& r) {
        // exactly ONE store instruction per tile and wave (sample 0 of every tile exists): the vmcnt bookkeeping needs it
        const bool ok = sqs < nv;
        // (UNIT: no multiplicity of zero takes a sample beyond N out of the sums, and its column of P is zero only after
        // k_build_gram / k_make_p -- k_build_sweep normalises the zero energies of the padding like any sample's.  Its reciprocal
        // is zeroed instead: the same products w r = 0 and r sw = 0 as in the general kernel, once per tile rather than per group.)
        if constexpr (UNIT) r = ok ? r : 0.0;
        // The store is written out with its lane mask: a compiler-made `if (ok)` is a branch around it, and with a branch inside
        // the two-tile loop body the register allocator no longer holds the pinned accumulators in place.  (The compiler does not
        // count this store in its own vmcnt arithmetic; every wait of the loop is explicit, wait_vm.)  The reciprocal passes
        // THROUGH the statement: whatever reads it afterwards -- the DPP broadcasts of the next tile's first group, which need two
        // wait states after the vector instruction that wrote it and which the hazard recogniser cannot see -- stands behind
        // these three instructions.  (s_and_saveexec writes SCC: declared, or a loop test the compiler has formed in front of the
        // store is read behind it.)
        const uint64_t okm = __builtin_amdgcn_ballot_w64(ok);
        const uint64_t sb = reinterpret_cast<uint64_t>(rlo + tile * (TS * 8));
        uint64_t saved;
        if constexpr (WIDE) {
            const uint64_t a = sb + roff;
            asm volatile("s_and_saveexec_b64 %0, %2\n\tglobal_store_dwordx2 %3, %1, off\n\ts_mov_b64 exec, %0"
                         : "=&s"(saved), "+v"(r) : "s"(okm), "v"(a) : "memory", "scc");
        } else {
            asm volatile("s_and_saveexec_b64 %0, %2\n\tglobal_store_dwordx2 %3, %1, %4\n\ts_mov_b64 exec, %0"
                         : "=&s"(saved), "+v"(r) : "s"(okm), "v"(roff), "s"(sb) : "memory", "scc");
        }
    };
    // One 1 KB piece of a tile, the pieces of a tile in ascending order.  The lane offsets are laundered IN PLACE (stage_piece
    // launders a copy, which costs a move per parity and tile in this loop).  ub: the piece's wave-uniform source; panels without a
    // live mask step it from piece to piece by the one pitch of eight rows -- as 8 j ld + column it keeps a loop-invariant
    // register pair per piece alive, which the scalar file of the two-tile loop no longer has.
    const uint64_t pitch8 = (uint64_t)ld * 64;
    auto request_piece = [&](int j, int64_t tile, char* dst, uint64_t& ub) {
        if constexpr (NB <= 2)
            ub = reinterpret_cast<uint64_t>(P + rows(8 * j) * ld + rows.cols(j, tile * TS));
        else
            ub = j == 0 ? reinterpret_cast<uint64_t>(P + tile * TS) : ub + pitch8;
        if constexpr (WIDE) {
            asm("" : "+s"(ub));
            stage_piece<true>(reinterpret_cast<const double*>(ub), so.off[j & 1], dst, lane);
        } else {
            asm("" : "+s"(ub));
            asm("" : "+v"(so.off[j & 1]));
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(reinterpret_cast<const char*>(ub) + so.off[j & 1]),
                                             (__attribute__((address_space(3))) void*)dst, 16, 0, MBAR_DMA_AUX);
        }
    };
    // Software pipeline over the wave's tiles t_0, t_1, ... (two LDS buffers): while the Gram blocks of tile t_i issue, the
    // 4x4x4 blocks of tile t_{i+1}'s normalisers are slipped in between them (their LDS operands requested a row of blocks
    // earlier), the Gram operands are fetched one group ahead, and tile t_{i+2} is requested into t_i's buffer as soon as
    // its last group has been read -- no LDS round trip and no HBM latency is left exposed in the loop.
    //   vmcnt, in issue order, at the top of iteration i: [tile t_{i+1}: NDMA] [store of tile t_i's reciprocals: 1]
    // The loop's bookkeeping is 32-bit and scalar (the launcher refuses ntiles >= 2^31, far beyond any device's memory): left =
    // ntiles - t counts the matrix's tiles from the wave's current one on, so that tile t + k W exists while left > k Wn, and is
    // the matrix's last -- the only one that can be ragged -- when left - k Wn = 1.  (A 64-bit comparison has no scalar form.)
    int64_t t = gw;
    const int Wn = (int)W;
    int left = (int)(ntiles - gw);
    auto count_of = [&](int l) { return l > 1 ? TS : (l == 1 ? nlast : 0); };  // samples of the tile that has l tiles from it on
    double rcur = 0.0;
    double uv[2][NB], w[2], sw[2];
    int first = 0;  // the buffer of the wave's first tile: 1 when the wave has an odd number of tiles (see the loop)
    if (left > 0) {
        first = (int)(((uint32_t)(left - 1) / (uint32_t)Wn + 1u) & 1u);
        const int fb = first * TILE_BYTES;
        stage(t, buf + fb);
        if (left > Wn) {
            stage(t + W, buf + (TILE_BYTES - fb));
            wait_vm<NDMA>();
        } else {
            wait_vm<0>();
        }
        double sa = 0.0, sb = 0.0;
#pragma unroll
        for (int st = 0; st < NSTEP; st += 2) {
            double a0, b0, a1, b1;
            read_step(fb, st, a0, b0);
            read_step(fb, st + 1, a1, b1);
            sa = __builtin_amdgcn_mfma_f64_4x4x4f64(a0, b0, sa, 0, 0, 0);
            sb = __builtin_amdgcn_mfma_f64_4x4x4f64(a1, b1, sb, 0, 0, 0);
        }
        // (a padded sample has an all-zero column: keep its reciprocal finite, its multiplicity is 0)
        rcur = recip_fast(fmax(sa + sb, 1e-300));
        store_rinv(t, count_of(left), rcur);
        read_group(fb, 0, uv[0], w[0], sw[0]);
    }
    // One tile of the pipeline, out of buffer CUR of the wave's pair.  The loop below runs two per trip, buffer 0 then buffer 1, so
    // that every LDS address is a loop-invariant lane register + an immediate.  A wave with an odd number of tiles enters the
    // first trip at its second half -- which is why its first tile went to buffer 1 above: a third copy of the body behind the
    // loop for an odd LAST tile costs the pinned accumulators their registers (moves and scratch), a skipped first half does not.
    // (CUR is a literal at both calls and the body is inlined there: a generic lambda with a constant parameter type would say
    // so outright, but the asm operands G[b] below do not survive one)
    auto tile_step = [&](const int CUR) __attribute__((always_inline)) {
        const int CB = CUR * TILE_BYTES, NXB = (CUR ^ 1) * TILE_BYTES;
        char* cbuf = buf + CB;
        const int64_t tn = t + W, tnn = t + 2 * W;
        const int64_t tstage = left > 2 * Wn ? tnn : t;
        uint64_t piece_src = 0;
        // (the multiplier table never changes: without this the compiler keeps all of it in 8 NB registers)
        if constexpr (!UNIT) asm volatile("" : "+v"(cop_off));
        // (four accumulators in rotation: the asm 4x4x4 blocks are invisible to the hazard recogniser, and a dependent one
        // needs four wait states after its predecessor)
        double sacc[4];
        [[maybe_unused]] double r1n = 0.0;
        // (the four groups are four inlined calls with a literal g, not an unrolled loop: two tiles per trip put the full panel's
        // unrolled groups at the size beyond which `#pragma unroll` is no longer honoured, and the Gram blocks G[b] then lose
        // their constant indices -- and their registers)
        auto group_step = [&](const int g) __attribute__((always_inline)) {
            const int gc = g & 1, gn = gc ^ 1;
            if (g == 2) wait_vm<1>();  // tile t_{i+1}, requested three quarters of an iteration ago
            // (UNIT: q0 = r0 exactly, so the first candidate's update takes the broadcast inside the fused multiply-add itself --
            // the same operation on the same operands, without the move)
            // r1 feeds a plain multiplication and keeps its move.  UNIT: groups 1-3 take it from r1n, moved a group EARLIER (in
            // front of the previous group's Gram blocks): the compiler does not count an asm statement as an instruction and pads
            // the first instruction it can see reading an asm result that is not a counted instruction away.
            double r0 = 0.0, r1;
            switch (g) {
                case 0: if constexpr (!UNIT) r0 = row16_bcast<0>(rcur); r1 = row16_bcast<1>(rcur); break;
                case 1: if constexpr (!UNIT) { r0 = row16_bcast<4>(rcur); r1 = row16_bcast<5>(rcur); } else { r1 = r1n; } break;
                case 2: if constexpr (!UNIT) { r0 = row16_bcast<8>(rcur); r1 = row16_bcast<9>(rcur); } else { r1 = r1n; } break;
                default: if constexpr (!UNIT) { r0 = row16_bcast<12>(rcur); r1 = row16_bcast<13>(rcur); } else { r1 = r1n; } break;
            }
            const double q0 = UNIT ? r0 : w[gc] * r0, q1 = UNIT ? r1 : w[gc] * r1;
#pragma unroll
            for (int I = 0; I < NB; ++I) {
                if constexpr (UNIT) {
                    switch (g) {
                        case 0: fmac_row16_bcast<0>(acc[0][I], rcur, uv[gc][I]); break;
                        case 1: fmac_row16_bcast<4>(acc[0][I], rcur, uv[gc][I]); break;
                        case 2: fmac_row16_bcast<8>(acc[0][I], rcur, uv[gc][I]); break;
                        default: fmac_row16_bcast<12>(acc[0][I], rcur, uv[gc][I]); break;
                    }
                } else {
                    acc[0][I] = fma(uv[gc][I], q0, acc[0][I]);
                }
                if constexpr (ACC1) acc[1][I] = fma(uv[gc][I], q1, acc[1][I]);
                // (pinned here: left alone, the compiler sinks all 8 NB updates to the end of the iteration and keeps
                // the operands of all four groups alive for them)
                settle(acc[0][I]);
                if constexpr (ACC1) settle(acc[1][I]);
            }
            // (a padded sample needs no mask: its multiplicity and the root of it are stored as zeros; UNIT: its reciprocal is)
            const double rin = UNIT ? r1 : r1 * sw[gc];  // operand of the Newton-Raphson candidate's Gram matrix
            double p[NB];
#pragma unroll
            for (int I = 0; I < NB; ++I) p[I] = uv[gc][I] * rin;
            if constexpr (UNIT) {
                switch (g) {
                    case 0: r1n = row16_bcast<5>(rcur); break;
                    case 1: r1n = row16_bcast<9>(rcur); break;
                    case 2: r1n = row16_bcast<13>(rcur); break;
                    default: break;
                }
            }
            // Operands of the next group and of the 4x4x4 steps this group carries (the next tile's normalisers ride on this
            // tile's groups 2 and 3: 2 NB steps each, their operands fetched in two batches of NB for wide panels), the weights'
            // piece of the tile after next: with pinned accumulators these are issued BEHIND the group's first Gram blocks
            // (request_next / request_steps below), otherwise here and the compiler places them.
            constexpr int B1 = NB >= 4 ? NB : 2 * NB;
            double opa[B1], opb[B1];
            auto request_next = [&]() {
                if (g < GROUPS - 1) {
                    read_group(CB, g + 1, uv[gn], w[gn], sw[gn]);
                } else {
                    // (every read of this tile was issued a group ago and has been consumed: its buffer can take the tile
                    // after next -- past the end this tile is simply requested again and never looked at, so that the loop
                    // body stays ONE basic block: the register allocator handles the 288 pinned accumulator registers only then)
                    read_group(NXB, 0, uv[gn], w[gn], sw[gn]);
                }
            };
            auto request_steps = [&]() {
                if (g >= 2) {
#pragma unroll
                    for (int q = 0; q < B1; ++q) read_step(NXB, (g - 2) * 2 * NB + q, opa[q], opb[q]);
                }
            };
            if constexpr (!PINNED) {
                request_next();
                request_steps();
            }
            auto mfma = [&](int b, double x, double y) {
                if constexpr (PINNED) {
                    if (b < GRAM_AGPR_BLOCKS)
                        asm volatile("v_mfma_f64_16x16x4_f64 %0, %1, %2, %0" : "+a"(G[b]) : "v"(x), "v"(y));
                    else
                        asm volatile("v_mfma_f64_16x16x4_f64 %0, %1, %2, %0" : "+v"(G[b]) : "v"(x), "v"(y));
                } else {
                    G[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, G[b], 0, 0, 0);
                }
            };
            if constexpr (PINNED) {  // (asm MFMAs are opaque to the scheduler and the hazard recogniser: see k_gram)
                __builtin_amdgcn_sched_barrier(0);
                asm volatile("s_nop 7");
            }
            constexpr int NM = NBLK;  // 16x16x4 instructions per group
            int b = 0, nm = 0;
#pragma unroll
            for (int I = 0; I < NB; ++I) {
                if (NB == 1 && g >= 2) {
                    mfma4(sacc[2 * (g & 1)], opa[0], opb[0], true);
                    mfma4(sacc[2 * (g & 1) + 1], opa[1], opb[1], true);
                }
#pragma unroll
                for (int J = I; J < NB; ++J) {
                    mfma(b, p[I], p[J]);
                    if constexpr (PINNED) {
                        if (nm == 0 || nm == 1) {
                            __builtin_amdgcn_sched_barrier(0);
                            if (nm == 0) request_next(); else request_steps();
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    }
                    if (g == GROUPS - 1) {  // pieces [nm NDMA / NM, (nm + 1) NDMA / NM) of the tile after next; the last = weights
#pragma unroll
                        for (int j = nm * NDMA / NM; j < (nm + 1) * NDMA / NM; ++j) {
                            if constexpr (PINNED) __builtin_amdgcn_sched_barrier(0);
                            if (j < ROWS / 8)
                                request_piece(j, tstage, cbuf + j * 1024, piece_src);
                            else if constexpr (!UNIT)
                                stage_w(tstage, cbuf);
                            if constexpr (PINNED) __builtin_amdgcn_sched_barrier(0);
                        }
                    }
                    ++b;
                    ++nm;
                }
                // 4x4x4 steps of the next tile after every row of blocks but the last (so that the accumulators are long
                // complete when the VALU reads them): fused_steps_done(I) of the group's 2 NB steps are issued by row I
                if (g >= 2 && NB > 1 && I < NB - 1) {
#pragma unroll
                    for (int q = fused_steps_done<NB>(I - 1); q < fused_steps_done<NB>(I); ++q)
                        mfma4(sacc[q & 3], opa[q % B1], opb[q % B1], g == 2 && q < 4);
                    if (B1 < 2 * NB && fused_steps_done<NB>(I - 1) < B1 && fused_steps_done<NB>(I) >= B1) {
#pragma unroll
                        for (int q = 0; q < B1; ++q) read_step(NXB, (g - 2) * 2 * NB + B1 + q, opa[q], opb[q]);
                    }
                }
            }
            if constexpr (PINNED) __builtin_amdgcn_sched_barrier(0);
        };
        static_assert(GROUPS == 4, "the tile loop names its four groups");
        group_step(0);
        group_step(1);
        group_step(2);
        group_step(3);
        // (the wait states between the last 4x4x4 block and the VALU reading its result; tied to the accumulators so that the
        // scheduler cannot move the additions in front of it)
        if constexpr (PINNED)
            asm volatile("s_nop 7\n\ts_nop 7" : "+v"(sacc[0]), "+v"(sacc[1]), "+v"(sacc[2]), "+v"(sacc[3]));
        rcur = recip_fast(fmax((sacc[0] + sacc[1]) + (sacc[2] + sacc[3]), 1e-300));
        store_rinv(tn, count_of(left - Wn), rcur);  // (past the wave's last tile the count is 0)
        t = tn;
        left -= Wn;
    };
    int skip = first;
    while (left > 0) {
        asm volatile("" : "+s"(skip));
        if (!skip) tile_step(0);
        skip = 0;
        tile_step(1);
    }
    if constexpr (PINNED) asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
#pragma unroll
    for (int f = 0; f < 2; ++f) {
#pragma unroll
        for (int I = 0; I < NB; ++I) {
            double v = acc[f][I];
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            if (lane < 16) psum_part[(gw * 2 + f) * ROWS + 16 * I + lane] = v;
        }
    }
    {
        int b = 0;
#pragma unroll
        for (int I = 0; I < NB; ++I)
#pragma unroll
            for (int J = I; J < NB; ++J, ++b) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
#if defined(MBAR_GRAM_STORE_NT)  // (A/B build, profiles/r6_ab_fused_record_stores_nt.txt)
                    __builtin_nontemporal_store(G[b][r], &gram_part[((gw * NBLK + b) * 4 + r) * 64 + lane]);
#else
                    gram_part[((gw * NBLK + b) * 4 + r) * 64 + lane] = G[b][r];
#endif
                }
            }
    }
}


// ---------------------------------------------------------------------------------------------
// host-side launchers
// ---------------------------------------------------------------------------------------------

// Fused sweep (P mode): geometry of the full Gram panel -- one workgroup of four waves per CU, two tile buffers per wave.
// unit: the launch is k_fused<.., UNIT> (no weights' piece, no multiplier table in LDS); the grid -- and with it the partial
// records and the order of every sum -- is that of the general kernel, so that the two agree to the bit.
LaunchGeom fused_geometry(int nb, int num_cu, int64_t ntiles, int64_t grid_override, bool unit) {
    LaunchGeom g;
    g.waves = 4;
    g.variant = 1;
    if (nb > 8) {  // 129 .. 256 states: one tile stream per workgroup, one partial record per workgroup (k_fused_quad)
        g.variant = 6;
        g.lds_bytes = (size_t)2 * ((size_t)nb * 16 * TS * 8 + 4 * 1024) + 1024;
        int64_t capq = grid_override > 0 ? grid_override : num_cu;
        int64_t wantq = ntiles < 1 ? 1 : ntiles;
        g.blocks = (int)(wantq < capq ? wantq : capq);
        g.nwaves = g.blocks;
        g.psum_records = g.nwaves;
        return g;
    }
    const size_t tile = (size_t)nb * 16 * TS * 8 + 1024;    // + one LDS-DMA piece for the two weight vectors
    // The GRID is derived from the general kernel's LDS size in both forms (by_lds below): the unit form needs less, but a grid
    // of its own would change the partial records and the order of the sums, and the two forms would no longer agree to the bit.
    const size_t lds_general = (size_t)4 * 2 * tile + (size_t)nb * 512;  // + the candidates' multipliers as a 4x4x4 MFMA operand
    g.lds_bytes = unit ? (size_t)4 * 2 * (tile - 1024) : lds_general;    // what the launch asks for
    int64_t want = (ntiles + 3) / 4;
    int64_t cap = num_cu;
    if (nb <= 5) {  // narrow panels: few accumulators, several workgroups per CU (cf. gram_geometry)
        static const int occ[6] = {1, 4, 4, 3, 2, 2};
        const int by_lds = blocks_per_cu_for(lds_general);
        cap = (int64_t)num_cu * (by_lds < occ[nb] ? by_lds : occ[nb]);
        // ... but every wave leaves a partial record (NB (NB + 1) / 2 blocks of 2 KB + the per-state sums) and pays a prologue:
        // a second workgroup per CU only once a wave has ~32 tiles to work on (config 5, K = 40, N = 95 000: 58 instead of
        // 64 us per iteration with one workgroup per CU; K = 32, N = 1e6 is fastest at two)
        int64_t by_work = (ntiles + 127) / 128;
        if (by_work < num_cu) by_work = num_cu;
        if (cap > by_work) cap = by_work;
    }
    if (grid_override > 0) cap = grid_override;
    if (want < 1) want = 1;
    g.blocks = (int)(want < cap ? want : cap);
    g.nwaves = g.blocks * 4;
    g.psum_records = g.nwaves;
    return g;
}
template <int NB>
static hipError_t launch_fused_nb(hipStream_t s, const LaunchGeom& g, const double* P, int64_t ld, int64_t N, const double* cmul,
                                  const double* cw, const double* wsq, bool unit, double* rinv0, double* gp, double* pp, const LoopCtl& lc) {
    auto go = [&](auto kern) -> hipError_t {
        if (g.lds_bytes > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds_bytes);
            if (e != hipSuccess) return e;
        }
        const int64_t ntiles = (N + TS - 1) / TS;
        if (ntiles > INT32_MAX) return hipErrorInvalidValue;  // (the tile loop counts in 32 bits)
        double* r1 = nullptr;
        if (lc.ev_start && lc.ev_stop)
            hipExtLaunchKernelGGL(kern, dim3(g.blocks), dim3(256), g.lds_bytes, s, lc.ev_start, lc.ev_stop, 0, P, ld, N, ntiles, cmul,
                                  cw, wsq, rinv0, r1, gp, pp, lc.ctl, lc.slot_stride);
        else
            hipLaunchKernelGGL(kern, dim3(g.blocks), dim3(256), g.lds_bytes, s, P, ld, N, ntiles, cmul, cw, wsq, rinv0, r1, gp, pp,
                               lc.ctl, lc.slot_stride);
        return hipGetLastError();
    };
    // (WIDE also when the distance between two slot vectors, the lane offset of the reciprocal stores, does not fit 32 bits)
    const bool wide = stage_offsets_wide(ld) || (uint64_t)lc.slot_stride * 16u + 128u >= (1ull << 32);
    if (unit) return wide ? go(k_fused<NB, true, true>) : go(k_fused<NB, false, true>);
    return wide ? go(k_fused<NB, true, false>) : go(k_fused<NB, false, false>);
}
hipError_t launch_fused(hipStream_t s, int nb, const LaunchGeom& g, const double* P, int64_t ld, int64_t N, const double* cmul,
                        const double* cw, const double* wsq, bool unit, double* rinv_base, double* gram_part, double* psum_part,
                        const LoopCtl& lc) {
    if (!lc.ctl) return hipErrorInvalidValue;  // (the slot vectors are addressed through the control words)
    if (nb == 12 || nb == 16) return launch_fused_quad(s, nb, g, P, ld, N, cmul, cw, wsq, rinv_base, gram_part, psum_part, lc);
    switch (nb) {
#define MBAR_CASE(NB_) \
    case NB_: return launch_fused_nb<NB_>(s, g, P, ld, N, cmul, cw, wsq, unit, rinv_base, gram_part, psum_part, lc);
        MBAR_CASE(1) MBAR_CASE(2) MBAR_CASE(3) MBAR_CASE(4) MBAR_CASE(5) MBAR_CASE(6) MBAR_CASE(7) MBAR_CASE(8)
#undef MBAR_CASE
        default: return hipErrorInvalidValue;
    }
}

}  // namespace mbar
