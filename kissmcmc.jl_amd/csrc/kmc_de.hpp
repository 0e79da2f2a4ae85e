// kmc_de.hpp -- the differential-evolution move (KMC_MOVE_DE, opt-in; ter Braak 2006, emcee's DEMove): the DE forms of the two
// half-step kernels of kmc_kernels.hpp.  DESIGN.md section 2 (the stream) and section 4a (the kernels).
//
//   half_step_de_vec<Dens, L, K, ITER, RAGGED>  the vector kernel's layout, front parameters, moment fold and write-through stores
//       (kmc_kernels.hpp: half_step_vec_body, whose comments apply here), with two partner rows read coalesced right after block 0 of
//       Philox; no draw ring; one GPU, double rows, no blobs.
//   half_step_de_generic<Dens>                  one walker per lane, any ndim; the host route's PROPOSE / ACCEPT passes too.
//
// The stretch kernels are left exactly as they are: this header only adds kernels.
#pragma once
#include "kmc_kernels.hpp"

namespace kmc {

// Differential-evolution move (KMC_MOVE_DE, opt-in): its own Philox stream, key {seed_lo ^ "DEMV", seed_hi},
// counter {step_lo, step_hi, walker, block}.  Block 0: partners j, k (distinct, uniform over the complementary half) and the accept
// uniform; block 1: the jitter of gamma.  The kernels reuse Draw: partner = j, z = gamma of this step, t1 unused, lu = log u.
// DrawConsts carries gamma0 in c0 and sigma in c1 for a DE sampler (kmc_launch.hip: make_args).  log u is log_pos_normal (u in [2^-53, 1)).
constexpr uint32_t kDeKey = 0x44454D56u;   // "DEMV"
__device__ __forceinline__ U4 de_bits(uint32_t seed_lo, uint32_t seed_hi, uint64_t step, uint32_t walker, uint32_t block)
{
    return philox4x32_10((uint32_t)step, (uint32_t)(step >> 32), walker, block, seed_lo ^ kDeKey, seed_hi);
}
// the second partner: uniform over the h - 1 walkers other than j
__device__ __forceinline__ uint32_t de_partner_k(uint32_t w1, uint32_t nhalf, uint32_t j)
{
    const uint32_t k = __umulhi(w1, nhalf - 1u);
    return k + (k >= j ? 1u : 0u);
}
__device__ __forceinline__ double de_accept_u(const U4& w)
{
    const uint64_t k = ((uint64_t)w.z << 20) | (uint64_t)(w.w >> 12);
    return ((double)k + 0.5) * 0x1.0p-52;
}
// gamma = gamma0 (1 + sigma v), v uniform in (-1, 1): separately rounded operations, no fma
__device__ __forceinline__ double de_gamma(const DrawConsts& dc, uint32_t b1x)
{
    const double v = 2.0 * (((double)b1x + 0.5) * 0x1.0p-32) - 1.0;
    return dc.c0 * (1.0 + dc.c1 * v);
}
__device__ __forceinline__ Draw de_draw(const DrawConsts& dc, uint64_t step, uint32_t walker, uint32_t* partner_k)
{
    const U4 w = de_bits(dc.seed_lo, dc.seed_hi, step, walker, 0u);
    const U4 v = de_bits(dc.seed_lo, dc.seed_hi, step, walker, 1u);
    Draw d;
    d.partner = __umulhi(w.x, dc.nhalf);
    *partner_k = de_partner_k(w.y, dc.nhalf, d.partner);
    d.z = de_gamma(dc, v.x);
    d.t1 = 0.0;
    d.lu = log_pos_normal(de_accept_u(w));
    return d;
}
// a symmetric move: p1 - p0 >= log u, no (N-1) log z term
__device__ __forceinline__ bool de_accept_test(const Draw& d, double p1, double p0)
{
    return (p1 - p0) >= d.lu;
}

// ------------------------------------------------------------------------------------------
// Vector kernel.
// ------------------------------------------------------------------------------------------
// RAGGED = false: ndim == 2*L*K exactly; RAGGED = true: ndim < 2*L*K, as half_step_vec_body.
template <class Dens, int L, int K, int ITER, bool RAGGED>
__device__ __forceinline__ void half_step_de_vec_body(const HalfStepFront& f, const HalfStepArgs& a)
{
    static_assert(L >= 1 && L <= 64 && (L & (L - 1)) == 0, "L must be a power of two <= 64");
    static_assert(BlobTrait<Dens>::n == 0, "no blobs with the DE move (kmc_validate)");
    using T = double;
    using V2 = double2;                                 // one chunk = two consecutive elements of a row
    double* const posT = f.pos;
    static_assert(ITER >= 1 && ITER <= L, "a group's scalar lanes must cover its iterations");
    constexpr int G = 64 / L;          // groups = walkers in flight per wave
    constexpr int W = G * ITER;        // walkers per wave
    // Ragged rows: the row stride stands in front of the very first loads and ndim in front of the log-density.  Read from the argument struct they cost a scalar round
    // trip each where the compiler happens to put the wait (measured: in front of the own rows, and again -- sharing a counter with ds_bpermute -- in front of the partner
    // rows) that the exact-size kernels do not pay: everything in front of THEIR loads is a preloaded parameter.  So ndim travels among the preloaded parameters too, in the
    // 16 bits above a device address (kmc_launch.hip: front_of packs it for exactly these kernels); ld = ndim rounded up to even (kmc_sampler_create).
    // (pointer arithmetic, not an integer cast back: the loads stay global_load -- a flat_load would count on lgkmcnt and stall the scalar pipeline's waits)
    const uint64_t ndim_tag = RAGGED ? reinterpret_cast<uint64_t>(f.logp) >> 48 : 0ull;
    double* const logp_p = RAGGED ? reinterpret_cast<double*>(reinterpret_cast<char*>(f.logp) - (ndim_tag << 48)) : f.logp;
    const int ndim = RAGGED ? (int)ndim_tag : 2 * L * K;
    const int64_t ld = RAGGED ? (int64_t)((ndim + 1) & ~1) : (int64_t)(2 * L * K);
    const int tid   = blockIdx.x * vec_tpb(L) + threadIdx.x;
    const int lane  = threadIdx.x & 63;
    const int j     = lane & (L - 1);
    const int g     = lane / L;
    const int gbase = lane & ~(L - 1);                  // first lane of this group
    const int w0    = (tid >> 6) * W;                   // first active index of this wave
    const int nact  = f.n_active();
    const int half  = f.half();
    const int64_t own_row0 = (int64_t)f.gw0;                            // row of active walker 0 in pos / logp / naccept
    bool cv[K];                                         // chunk k of this lane lies inside the row
#pragma unroll
    for (int k = 0; k < K; ++k) cv[k] = !RAGGED || 2 * (k * L + j) < (int)ld;
    // Ragged rows are loaded AND stored without masks: a lane whose chunk lies past the row's end works on the row's LAST chunk instead (same cache line; no exec-mask
    // region around every load and store, nothing to zero).  It then computes what the chunk's real lane computes, from the same inputs, and stores the same bits to the
    // same address; what it holds never counts -- the densities select by element index against ndim, the moment read-out stops at ndim.
    // Row offsets: rows < 2^31 and ld < 2^31, one 32 x 32 -> 64 multiply instead of the 64-bit product.
    int ck[K];
#pragma unroll
    for (int k = 0; k < K; ++k) ck[k] = cv[k] ? k * L + j : (int)(ld >> 1) - 1;
    auto row_off = [&](int64_t row) -> int64_t { return RAGGED ? (int64_t)((uint64_t)(uint32_t)row * (uint64_t)(uint32_t)ld) : row * ld; };
    KMC_STAMP(0);                                       // wave entry

    // ---- scalar layout: one walker per lane.  Lane (g, j), j < ITER, carries walker slot j of its group and feeds this launch; the
    //      other lanes of the group draw for a clamped walker and are never used (the stretch kernel parks future steps there) --------
    const int64_t oth_row0 = (int64_t)(1 - half) * (int64_t)f.nhalf;
    const int  jq     = j / ITER, js = j - jq * ITER;
    const bool useA   = jq == 0;
    const int  iA     = w0 + js * G + g;
    const bool validA = useA && (iA < nact);
    const int      iAc = iA < nact ? iA : nact - 1;
    const int64_t  rowA = own_row0 + iAc;                                // row in pos / index in logp, naccept

    // ---- row layout: own rows of every iteration (independent of the random draws) ----------
    bool    validB[ITER];
    double2 xc[ITER][K], xo[ITER][K];
    double2 xk[ITER][K];                                                // the second partner's rows (xo: the first's, then the proposal)
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const int i = w0 + it * G + g;
        validB[it] = i < nact;
        const V2* own = reinterpret_cast<const V2*>(posT + row_off(own_row0 + (validB[it] ? i : nact - 1)));
#pragma unroll
        for (int k = 0; k < K; ++k) xc[it][k] = load_row(&own[ck[k]]);
    }

    // ---- the walker's log-pdf and counters: same block, addressed from the preloaded parameters alone -------------
    const int64_t nrows_blk = 2 * (int64_t)f.nhalf;
    uint32_t* const naccept_p = reinterpret_cast<uint32_t*>(logp_p + nrows_blk);
    uint32_t* const klast_p = naccept_p + nrows_blk;
    const double   p0 = logp_p[rowA];
    const uint32_t na = naccept_p[rowA];
    const uint32_t kl = klast_p[rowA];

    // ---- the step, then Philox: nothing here touches the argument struct.  Eager launch: the step is a preloaded
    //      parameter, so the partner index is known without any memory access; graph replay: one scalar round trip
    //      for the schedule entry (the struct's fields ride the same round trip, see below) -----------------------
    const bool eager = f.sched == nullptr;
    SchedEntry sch_t{0, 0, 0u, 0u, {0u, 0u}};
    if (!eager) sch_t = schedule_entry(f);
    const uint64_t step = eager ? (uint64_t)f.step : 2ull * (uint64_t)sch_t.gen + (uint64_t)half;
    // block 0: both partners and the accept uniform -- all the partner-row loads need
    const U4 bits = de_bits(f.seed_lo, f.seed_hi, step, f.gw0 + (uint32_t)iAc, 0u);
    const uint32_t partnerA = __umulhi(bits.x, f.nhalf);
    const uint32_t partnerK = de_partner_k(bits.y, f.nhalf, partnerA);
    KMC_STAMP(1);                                       // Philox done: the partner index is known

    // ---- scalar -> row: the partners of slot it*G+g live in lane gbase+it.  As in the stretch kernel, the partner-row loads of the first
    //      half of the iterations go out before block 1 of Philox and the logarithm, the rest after them ----------------------------------
    auto load_partner_rows = [&](int it) {
        const uint32_t pj = (uint32_t)__builtin_amdgcn_ds_bpermute((gbase + it) * 4, (int)partnerA);
        const uint32_t pk = (uint32_t)__builtin_amdgcn_ds_bpermute((gbase + it) * 4, (int)partnerK);
        const double2* othj = reinterpret_cast<const double2*>(f.pos + row_off(oth_row0 + pj));
        const double2* othk = reinterpret_cast<const double2*>(f.pos + row_off(oth_row0 + pk));
#pragma unroll
        for (int k = 0; k < K; ++k) xo[it][k] = load_row(&othj[ck[k]]);
#pragma unroll
        for (int k = 0; k < K; ++k) xk[it][k] = load_row(&othk[ck[k]]);
    };
    constexpr int kFirst = ITER >= 2 ? ITER / 2 : ITER;                 // iterations whose loads precede the first logarithm
#pragma unroll
    for (int it = 0; it < kFirst; ++it) load_partner_rows(it);
    __builtin_amdgcn_sched_barrier(0);
    KMC_STAMP(2);                                       // the first partner-row loads are issued

    // ---- from here on the argument struct: one scalar round trip for all of it (have every field the kernel
    //      uses later requested by now, otherwise the compiler fetches some lazily: a round trip each) ----------
    asm volatile("" :: "s"(a.chain), "s"(a.chain_logp), "s"(a.chain_rows), "s"(a.chain_row0),
                 "s"(a.msum), "s"(a.msumsq), "s"(a.macc_stride), "s"(a.sched_inline.gen), "s"(a.sched_inline.slot),
                 "s"(a.sched_inline.flags), "s"(a.sched_inline.nbefore));
    // (the launch kind again, opaque to the optimiser: merged with the branch above it would pull the struct's first
    //  use -- and the wait for it -- in front of Philox)
    int eager_late = eager ? 1 : 0;
    asm volatile("" : "+v"(eager_late));
    eager_late = __builtin_amdgcn_readfirstlane(eager_late);
    SchedEntry sch = sch_t;
    if (eager_late != 0) sch = a.sched_inline;
    const bool count  = (sch.flags & kCount) != 0;
    const bool sample = (sch.flags & kSample) != 0;
    const DrawConsts dc = a.dc;                                         // gamma0 in c0, sigma in c1 (kmc_launch.hip: make_args)
    // Streaming moments are sojourn-weighted: a walker's value is credited, times the number of
    // samples it stood for, when it is replaced (and by flush_moments_vec at read-out).  Only waves
    // with an accepted move touch their accumulators -- at low acceptance (large ndim) almost none.
    const bool do_mom = count && a.msum != nullptr;
    // small rows: nearly every wave has an accepted move, so fetch its accumulator slots now and
    // keep that latency off the kernel's tail; large rows: fetch only when needed
    constexpr bool kPrefetchAcc = K <= 2 && L != 64;                   // L == 64: the moment ring instead (below)
    constexpr bool kMomRing = !kPrefetchAcc && !FoldT<L, K>::on && L == 64;          // HalfStepArgs::mring
    if constexpr (kMomRing) asm volatile("" :: "s"(a.mring), "s"(a.mring_w), "s"(a.mcnt), "s"(a.mswept), "s"(a.mring_depth));
    double2 accs[K], accq[K];
    double  acct[4] = {0.0, 0.0, 0.0, 0.0};
    // Large ensembles (ITER >= 4: the planner's choice from 16 384 waves on -- states that live in HBM) with several waves per workgroup: the
    // waves' sums are added up through LDS and ONE wave per workgroup reads and rewrites accumulator slots (its own; the others' stay as the
    // read-out and the flush kernel find them), in a fixed order -- a quarter (L = 32) or half (L = 8) of the accumulator bytes, which were 10 %
    // of a launch's HBM traffic at 524 288 x 128 (33.5 MB in + 33.5 MB out of 656 MB; profiles/traffic_hbm_512kx128.json).
    constexpr bool kWgFold = FoldT<L, K>::on && vec_tpb(L) > 64 && ITER >= 4;
    const bool acc_owner = !kWgFold || (threadIdx.x >> 6) == 0;
    if constexpr (FoldT<L, K>::on) {
        if (do_mom && acc_owner) {
#pragma unroll
            for (int r = 0; r < FoldT<L, K>::NVL; ++r) acct[r] = a.msum[((int64_t)(tid >> 6) * FoldT<L, K>::NVL + r) * 64 + lane];
        }
    } else if constexpr (kPrefetchAcc) {
        if (do_mom && g == 0) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int64_t idx = (int64_t)k * a.macc_stride + tid;
                accs[k] = reinterpret_cast<const double2*>(a.msum)[idx];
                accq[k] = reinterpret_cast<const double2*>(a.msumsq)[idx];
            }
        }
    }
    uint32_t ring_posted = 0u, ring_swept = 0u;
    if constexpr (kMomRing) {
        if (do_mom && a.mring != nullptr) { ring_posted = a.mcnt[tid >> 6]; ring_swept = a.mswept[tid >> 6]; }
    }
    KMC_STAMP(3);                                       // the argument struct has arrived (schedule entry, constants)
    Draw dr;                                                            // partner = j, z = gamma of this step, lu = log u
    dr.partner = partnerA;
    {                                                                   // block 1: the jitter of gamma
        const U4 b1 = de_bits(f.seed_lo, f.seed_hi, step, f.gw0 + (uint32_t)iAc, 1u);
        dr.z = de_gamma(dc, b1.x);
        dr.t1 = 0.0;
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int it = kFirst; it < ITER; ++it) load_partner_rows(it);
    __builtin_amdgcn_sched_barrier(0);
    dr.lu = log_pos_normal(de_accept_u(bits));
    KMC_STAMP(4);                                       // both logarithms done, every partner-row load issued
    double zB[ITER];
#pragma unroll
    for (int it = 0; it < ITER; ++it) zB[it] = bperm_f64((gbase + it) * 4, dr.z);

    // ---- DE move + log-pdf; xo becomes the proposal ----------------------------------------
    double myp1 = 0.0;
    constexpr int kRowND = RowEvalTrait<Dens>::n;                       // > 0: a function body over the whole proposal (see below)
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
#pragma unroll
        for (int k = 0; k < K; ++k) {                                   // :255
            xo[it][k].x = xc[it][k].x + zB[it] * (xo[it][k].x - xk[it][k].x);      // y = x + g (x_j - x_k), separately rounded
            xo[it][k].y = xc[it][k].y + zB[it] * (xo[it][k].y - xk[it][k].y);
        }
        if constexpr (MultiSumTrait<Dens>::n > 0) {                    // a function body feeding several sums over the elements
            double S[MultiSumTrait<Dens>::n];
            Dens::template frag_partial_n<L, K>(xo[it], j, ndim, a.dp, S);
#pragma unroll
            for (int q = 0; q < MultiSumTrait<Dens>::n; ++q) S[q] = group_sum<L>(S[q]);
            const double p1 = Dens::finish_n(S, a.dp);                   // :257
            myp1 = (j == it) ? p1 : myp1;
        } else if constexpr (kRowND == 0) {
            const double S  = group_sum<L>(Dens::template frag_partial<L, K>(xo[it], j, ndim, a.dp));
            const double p1 = Dens::finish(S, a.dp);                     // :257
            myp1 = (j == it) ? p1 : myp1;                               // row -> scalar, no traffic
        }
    }
    if constexpr (kRowND > 0) {
        // A caller's function body over the whole proposal (BodyDensity): rows are loaded, moved and stored lane-striped like
        // everybody's, and only the evaluation is per walker -- the wave's W proposals go through a per-wave LDS tile (row stride
        // 2 L K + 2 doubles: 16-byte aligned chunks) and the scalar-layout lane of each walker, the one that holds its draws and
        // runs its accept test, calls the body once on its row there (src/samplers.jl:257), elements in index order: the same
        // value, bit for bit, as the one-walker-per-lane kernels give.
        extern __shared__ __attribute__((aligned(16))) double vec_rows[];
        constexpr int TS = 2 * L * K + 2;
        double* tile = vec_rows + (size_t)(threadIdx.x >> 6) * (size_t)(W * TS);
#pragma unroll
        for (int it = 0; it < ITER; ++it) {
#pragma unroll
            for (int k = 0; k < K; ++k)
                *reinterpret_cast<double2*>(&tile[(it * G + g) * TS + 2 * (k * L + j)]) = xo[it][k];     // (a tile row is 2 L K + 2 wide: chunks past a ragged row's end land behind it, unread)
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (useA) myp1 = Dens::eval_row(&tile[(js * G + g) * TS], ndim, a.dp);  // (inlined: the body's x[i] become LDS reads of this lane's row)
    }

    KMC_STAMP(5);                                       // both rows have arrived, the proposal's log-pdf is reduced
    // ---- accept test in the scalar layout ---------------------------------------------------
    const bool acc = validA && de_accept_test(dr, myp1, p0);            // p1 - p0 >= log u
    const unsigned long long accmask = __ballot(acc);
    if (acc) {
        store_wt(&logp_p[rowA], myp1);                                  // :262
        if (count) store_wt(&naccept_p[rowA], na + 1u);                 // :265
        if (do_mom) store_wt(&klast_p[rowA], sch.nbefore);
    }
    const uint32_t wA = (acc && do_mom) ? sch.nbefore - kl : 0u;        // samples the replaced value stood for
    const bool any_w = __ballot(wA != 0u) != 0ull;
    if (sample && a.chain_logp != nullptr && validA)                    // :271
        store_wt(&a.chain_logp[sch.slot * a.chain_rows + a.chain_row0 + iA], acc ? myp1 : p0);

    KMC_STAMP(6);                                       // accept test done, per-walker scalars stored
    // ---- row layout again: store accepted proposals, samples, moments -----------------------
    double2 ms[K], mq[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { ms[k] = make_double2(0.0, 0.0); mq[k] = make_double2(0.0, 0.0); }
    // room for one entry per walker of the wave? (wave-uniform; kMomRing geometries have one group per wave)
    const bool use_ring = kMomRing && a.mring != nullptr && ring_posted - ring_swept + (uint32_t)ITER <= (uint32_t)a.mring_depth;
    uint32_t ring_new = 0u;
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const bool accB = ((accmask >> (gbase + it)) & 1ull) != 0;
        if (accB) {                                                     // :261
            V2* own = reinterpret_cast<V2*>(posT + row_off(own_row0 + w0 + it * G + g));
#pragma unroll
            for (int k = 0; k < K; ++k) store_row(&own[ck[k]], xo[it][k]);
        }
        if (any_w) {
            const double wB = (double)(uint32_t)__builtin_amdgcn_ds_bpermute((gbase + it) * 4, (int)wA);
            if (use_ring) {
                if (wB != 0.0) {                                          // wave-uniform (L == 64: one group)
                    const int64_t e = (int64_t)(tid >> 6) * a.mring_depth + (int64_t)((ring_posted + ring_new) % (uint32_t)a.mring_depth);
                    double2* slot = a.mring + e * K * 64 + lane;
#pragma unroll
                    for (int k = 0; k < K; ++k) slot[k * 64] = xc[it][k];
                    if (lane == 0) a.mring_w[e] = wB;
                    ring_new += 1u;
                }
            } else {
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    ms[k].x += xc[it][k].x * wB; ms[k].y += xc[it][k].y * wB;
                    mq[k].x += (xc[it][k].x * xc[it][k].x) * wB; mq[k].y += (xc[it][k].y * xc[it][k].y) * wB;
                }
            }
        }
        if (sample && a.chain != nullptr && validB[it]) {               // :268-269
            V2* dst = reinterpret_cast<V2*>(reinterpret_cast<T*>(a.chain) + (sch.slot * a.chain_rows + a.chain_row0 + w0 + it * G + g) * ld);
#pragma unroll
            for (int k = 0; k < K; ++k) store_row(&dst[ck[k]], sel2(accB, xo[it][k], xc[it][k]));
        }
    }
    if constexpr (kWgFold) {
        if (do_mom) {                                                   // (uniform over the launch: every wave of the workgroup arrives)
            constexpr int NVL = FoldT<L, K>::NVL, NWV = vec_tpb(L) / 64;
            __shared__ double wg_fold[NWV - 1][NVL][64];
            const int wv = (int)(threadIdx.x >> 6);
            double v[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            if (any_w) fold_scatter<L, K>(lane, ms, mq, v);
            if (wv != 0) {
#pragma unroll
                for (int r = 0; r < NVL; ++r) wg_fold[wv - 1][r][lane] = v[r];
            }
            lds_barrier();
            if (wv == 0) {
                double* slot = a.msum + ((int64_t)(tid >> 6) * NVL) * 64 + lane;
#pragma unroll
                for (int r = 0; r < NVL; ++r) {
                    double t = v[r];
#pragma unroll
                    for (int w = 0; w < NWV - 1; ++w) t += wg_fold[w][r][lane];
                    store_wt(&slot[r * 64], acct[r] + t);
                }
            }
        }
    } else if (any_w) {
        if (use_ring) {
            if (lane == 0) a.mcnt[tid >> 6] = ring_posted + ring_new;
        } else {
            if constexpr (kPrefetchAcc) accumulate_wave<L, K, true>(a.msum, a.msumsq, a.macc_stride, tid, g, ms, mq, accs, accq, acct);
            else accumulate_wave<L, K, false>(a.msum, a.msumsq, a.macc_stride, tid, g, ms, mq, accs, accq, acct);
        }
    }
    KMC_STAMP(7);                                       // the last store is issued
}


template <class Dens, int L, int K, int ITER, bool RAGGED>
__global__ __launch_bounds__(vec_tpb(L)) void half_step_de_vec(KMC_FRONT_PARAMS, const HalfStepArgs a)
{
    half_step_de_vec_body<Dens, L, K, ITER, RAGGED>(KMC_FRONT_PACK, a);
}

// ------------------------------------------------------------------------------------------
// Generic kernel: one walker per lane, any ndim.
// ------------------------------------------------------------------------------------------
template <class Dens>
__device__ __forceinline__ void half_step_de_generic_body(const HalfStepFront& f, const HalfStepArgs& a)
{
    static_assert(BlobTrait<Dens>::n == 0, "no blobs with the DE move (kmc_validate)");
    const int tid = blockIdx.x * 256 + threadIdx.x;
    const SchedEntry sch = schedule_of(f, a);
    const uint64_t step = 2ull * (uint64_t)sch.gen + (uint64_t)a.half;      // (eager: sched_inline.gen)
    if (tid >= a.n_active) return;
    const int ndim = a.ndim;
    const bool count  = (sch.flags & kCount) != 0;
    const bool sample = (sch.flags & kSample) != 0;
    const int64_t gw = a.own_row0 + tid;                                // row in pos / index in logp, naccept
    uint32_t partner_k = 0u;
    const Draw dr = de_draw(a.dc, step, (uint32_t)(a.gw0 + tid), &partner_k);   // partner = j, z = gamma, lu = log u
    const int64_t ld = a.ld;
    double* own = a.pos + gw * ld;
    const double* oth = a.pos + (a.oth_row0 + dr.partner) * ld;         // x_j
    const double* othk = a.pos + (a.oth_row0 + partner_k) * ld;         // x_k
    const double p0 = a.logp[gw];
    constexpr bool kHost = HostEvalTrait<Dens>::value;
    if constexpr (kHost) {
        if (a.prop_out != nullptr) {                                    // PROPOSE pass
            for (int d = 0; d < ndim; ++d) a.prop_out[(int64_t)tid * a.prop_ld + d] = own[d] + dr.z * (oth[d] - othk[d]);
            return;
        }
    }
    typename Dens::Seq q;
    Dens::seq_init(q);
    for (int d = 0; d < ndim; ++d) {
        const double y = own[d] + dr.z * (oth[d] - othk[d]);             // y = x + g (x_j - x_k), separately rounded
        Dens::seq_add(q, y, d, a.dp);
    }
    double p1 = Dens::seq_finish(q, ndim, a.dp);                         // :257
    if constexpr (kHost) p1 = a.p1_in[tid];
    const bool acc = de_accept_test(dr, p1, p0);                        // p1 - p0 >= log u
    if constexpr (kHost) { if (a.acc_out != nullptr) a.acc_out[tid] = acc ? 1 : 0; }

    const bool do_mom = sample && a.msum != nullptr;
    const bool do_chain = sample && a.chain != nullptr;
    const int64_t row = sch.slot * a.chain_rows + a.chain_row0 + tid;
    if (acc || do_mom || do_chain) {
        for (int d = 0; d < ndim; ++d) {
            const double xcd = own[d];
            const double cur = acc ? xcd + dr.z * (oth[d] - othk[d]) : xcd;
            if (acc) own[d] = cur;                                      // :261
            if (do_chain) a.chain[row * ld + d] = cur;                  // :269
            if (do_mom) {
                const int64_t idx = (int64_t)d * a.macc_stride + tid;
                a.msum[idx] += cur;
                a.msumsq[idx] += cur * cur;
            }
        }
    }
    if (acc) {
        a.logp[gw] = p1;                                                // :262
        if (count) a.naccept[gw] += 1u;                                 // :265
    }
    if (sample && a.chain_logp != nullptr) a.chain_logp[row] = acc ? p1 : p0;   // :271
}

template <class Dens>
__global__ __launch_bounds__(256) void half_step_de_generic(KMC_FRONT_PARAMS, const HalfStepArgs a)
{
    half_step_de_generic_body<Dens>(KMC_FRONT_PACK, a);
}

}  // namespace kmc
