// kmc_shared_draws.hpp -- the exact-size stretch half-step of burn-in with ONE draw pass per workgroup (gfx950, wave64).
//
// half_step_vec's per-walker scalar pass -- Philox4x32-10, the partner index, z, (N-1) log z and log u -- runs in the scalar layout, where only
// ITER of a group's L lanes carry a walker: every wave issues the whole instruction stream for W = (64 / L) * ITER walkers.  Here a workgroup is
// SHARE waves and ONE of them (the leader) runs that pass once, with SHARE * ITER of every L lanes busy, for all SHARE * W walkers of the workgroup;
// the results reach their waves through LDS behind two workgroup barriers:
//   leader lane (g, j) draws for sibling wave v = j / ITER, walker slot (j % ITER) * G + g of that wave;
//   barrier 1 -- the partner indices are in LDS: every wave reads its own (in place of ds_bpermute) and requests its partner rows, in half_step_vec's
//                pinned order (first half of the iterations, then the leader's first logarithm, then the rest);
//   barrier 2 -- z, (N-1) log z and log u are in LDS: z goes to the row layout (in place of bperm_f64), the other two to the scalar lanes' accept test.
// A wave passes barrier 2 with all of its loads requested.  The global wave index keeps half_step_vec's meaning, so wave -> walkers and every address
// are unchanged; the arithmetic per walker, its order and every store are those of half_step_vec_body: results are the generic kernel's bit for bit.
// Control flow is uniform per wave and every wave of the (exactly full) grid reaches both barriers.
//
// Like the Credit instance (kmc_kernels.hpp: Spec) this is the eager form on a grid that is exactly full, for menu densities with a fragment form,
// double rows of exact size and one GPU -- but for BURN-IN: no generation of the launch is counted, sampled or credited, so the kernel reads and
// writes rows and log-pdfs only.  The host picks the kernel per replay (kmc_updated.hip: spec_of_chunk).  (The instance for counted replays was
// built and measured too, with two and with four waves per workgroup: 0.01 - 0.25 us per half-step SLOWER than the Credit instance at C2, so counted
// replays keep that one; profiles/NOTES.md.)
#pragma once
#include "kmc_tables.hpp"

namespace kmc {

// Workgroups per dispatch round, for the choice of the leader below: the CUs of an MI355X.  A tuning constant of C2's grid, not a contract.
constexpr int kShareRound = 256;

template <class Dens, int L, int K, int ITER, int SHARE>
__device__ __forceinline__ void half_step_share_body(const HalfStepFront& f, const HalfStepArgs& a)
{
    static_assert(BlobTrait<Dens>::n == 0 && RowEvalTrait<Dens>::n == 0, "menu densities with a fragment form");
    static_assert(ITER <= 2, "one or two walkers per group");
    static_assert(SHARE == 2 && SHARE * ITER <= L, "two waves per workgroup (the leader rule below is written for two); the leader's lanes must cover every sibling's walkers");
    constexpr int G = 64 / L;          // groups = walkers in flight per wave
    constexpr int W = G * ITER;        // walkers per wave
    constexpr int TPB = 64 * SHARE;
    constexpr int64_t ld = 2 * L * K;
    __shared__ uint32_t sh_partner[SHARE][W];
    __shared__ double sh_z[SHARE][W], sh_t1[SHARE][W], sh_lu[SHARE][W];
    double* const posT = f.pos;
    const int tid   = blockIdx.x * TPB + threadIdx.x;
    const int lane  = threadIdx.x & 63;
    const int wv    = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // this wave's place in the workgroup
    const int j     = lane & (L - 1);
    const int g     = lane / L;
    const int gbase = lane & ~(L - 1);                  // first lane of this group
    const int w0    = (tid >> 6) * W;                   // first active index of this wave
    const int half  = f.half();
    const int64_t own_row0 = (int64_t)f.gw0;
    const int64_t oth_row0 = (int64_t)(1 - half) * (int64_t)f.nhalf;
    // Which wave leads: a heuristic tuned at C2 (1024 workgroups of two waves on 256 CUs), nothing the results depend on.  ASSUMING that workgroups
    // reach the CUs in rounds of kShareRound and that a CU places the waves of successive workgroups on consecutive SIMDs, wave 0 leading everywhere
    // puts the leaders of a CU's four workgroups on two of its four SIMDs, where they contend for the VALU as before; with the leader alternating
    // every second round they sit on four.  The dispatch order is not documented and was not observed: what was measured is the period, 3.46 us per
    // burn-in half-step with this rule against 3.50 with wave 0 leading (generic kernel: 3.54).  Any choice gives the same results.
    const int lead = (int)(((unsigned)blockIdx.x / (2u * (unsigned)kShareRound)) & 1u);
    KMC_STAMP(0);                                       // wave entry

    // ---- scalar layout of THIS wave: lane (g, j) carries walker slot js = j % ITER of its group; the lanes with j < ITER run the accept test ----
    const int  js   = j % ITER;
    const bool useA = j < ITER;
    const int  iA   = w0 + js * G + g;
    const int64_t rowA = own_row0 + iA;

    // ---- row layout: own rows of every iteration, and the walker's log-pdf -- all addressed from the preloaded parameters, and in EVERY wave ahead
    //      of the draws.  (The leader's behind its Philox, to shorten what the siblings wait for, was measured: +0.1 us per half-step -- the rows'
    //      latency, not the instructions in front of Philox, is what the leader's own chain is made of.) ----
    double2 xc[ITER][K], xo[ITER][K];
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const double2* own = reinterpret_cast<const double2*>(posT + (own_row0 + w0 + it * G + g) * ld);
#pragma unroll
        for (int k = 0; k < K; ++k) xc[it][k] = load_row(&own[k * L + j]);
    }
    const double p0 = f.logp[rowA];

    // ---- the leader: Philox for the whole workgroup.  Lane (g, j) draws for wave vL, slot sL of that wave (lanes past the last sibling draw for a
    //      clamped wave and publish nothing) ----
    const int  vL   = j / ITER;
    const int  sL   = js * G + g;
    const bool pubL = vL < SHARE;
    const uint64_t step = (uint64_t)f.step;
    DrawConsts dcf{};
    dcf.seed_lo = f.seed_lo; dcf.seed_hi = f.seed_hi; dcf.nhalf = f.nhalf;
    U4 bits{0u, 0u, 0u, 0u};
    if (wv == lead) {
        const int iL = ((int)blockIdx.x * SHARE + (pubL ? vL : SHARE - 1)) * W + sL;
        bits = draw_bits(dcf, step, (uint64_t)f.gw0 + (uint64_t)iL);                  // RNG keyed by the GLOBAL walker index
        if (pubL) sh_partner[vL][sL] = draw_partner(dcf, bits);                       // :250
    }
    lds_barrier();                                      // barrier 1: the partner indices
    KMC_STAMP(1);                                       // the partner index is known

    auto load_partner_rows = [&](int it) {
        const uint32_t partner = sh_partner[wv][it * G + g];
        const double2* oth = reinterpret_cast<const double2*>(posT + (oth_row0 + partner) * ld);
#pragma unroll
        for (int k = 0; k < K; ++k) xo[it][k] = load_row(&oth[k * L + j]);
    };
    constexpr int kFirst = ITER >= 2 ? ITER / 2 : ITER;                 // iterations whose loads precede the first logarithm
#pragma unroll
    for (int it = 0; it < kFirst; ++it) load_partner_rows(it);
    __builtin_amdgcn_sched_barrier(0);
    KMC_STAMP(2);                                       // the first partner-row loads are issued

    // ---- from here on the argument struct (the draws' constants and the density's parameters): one scalar round trip ----
    DrawConsts dc = a.dc;
    dc.seed_lo = f.seed_lo; dc.seed_hi = f.seed_hi; dc.nhalf = f.nhalf;
    KMC_STAMP(3);
    double zL = 0.0, t1L = 0.0, luL = 0.0, ua = 0.5;
    if (wv == lead) {                                                   // the arithmetic of draw_finish, in two parts
        const double uz = ((double)bits.y + 0.5) * 0x1.0p-32;
        const double t  = fma(uz, dc.c1, dc.c0);
        zL = t * t;                                                     // :252
        const uint64_t kk = ((uint64_t)bits.z << 20) | (uint64_t)(bits.w >> 12);
        ua = ((double)kk + 0.5) * 0x1.0p-52;
        t1L = dc.nm1 * log_pos_normal(zL);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int it = kFirst; it < ITER; ++it) load_partner_rows(it);
    __builtin_amdgcn_sched_barrier(0);
    if (wv == lead) {
        luL = log_pos_normal(ua);                                       // :260
        if (pubL) { sh_z[vL][sL] = zL; sh_t1[vL][sL] = t1L; sh_lu[vL][sL] = luL; }
    }
    lds_barrier();                                      // barrier 2: z, (N-1) log z, log u; every partner-row load of this wave is out
    KMC_STAMP(4);
    Draw dr;
    dr.partner = 0u; dr.z = 0.0; dr.t1 = sh_t1[wv][js * G + g]; dr.lu = sh_lu[wv][js * G + g];
    double zB[ITER];
#pragma unroll
    for (int it = 0; it < ITER; ++it) zB[it] = sh_z[wv][it * G + g];

    // ---- stretch move + log-pdf; xo becomes the proposal ----
    double myp1 = 0.0;
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
#pragma unroll
        for (int k = 0; k < K; ++k) {                                   // :255
            xo[it][k].x = fma(zB[it], xc[it][k].x - xo[it][k].x, xo[it][k].x);
            xo[it][k].y = fma(zB[it], xc[it][k].y - xo[it][k].y, xo[it][k].y);
        }
        if constexpr (MultiSumTrait<Dens>::n > 0) {
            double S[MultiSumTrait<Dens>::n];
            Dens::template frag_partial_n<L, K>(xo[it], j, 2 * L * K, a.dp, S);
#pragma unroll
            for (int q = 0; q < MultiSumTrait<Dens>::n; ++q) S[q] = group_sum<L>(S[q]);
            const double p1 = Dens::finish_n(S, a.dp);                   // :257
            myp1 = (j == it) ? p1 : myp1;
        } else {
            const double S  = group_sum<L>(Dens::template frag_partial<L, K>(xo[it], j, 2 * L * K, a.dp));
            const double p1 = Dens::finish(S, a.dp);                     // :257
            myp1 = (j == it) ? p1 : myp1;                               // row -> scalar, no traffic
        }
    }
    KMC_STAMP(5);

    // ---- accept test in the scalar layout; burn-in: nothing is counted ----
    const bool acc = useA && accept_test(dr, myp1, p0);                 // :260
    const unsigned long long accmask = __ballot(acc);
    if (acc) store_wt(&f.logp[rowA], myp1);                             // :262
    KMC_STAMP(6);

    // ---- row layout again: store accepted proposals ----
#pragma unroll
    for (int it = 0; it < ITER; ++it) {
        const bool accB = ((accmask >> (gbase + it)) & 1ull) != 0;
        if (accB) {                                                     // :261
            double2* own = reinterpret_cast<double2*>(posT + (own_row0 + w0 + it * G + g) * ld);
#pragma unroll
            for (int k = 0; k < K; ++k) store_row(&own[k * L + j], xo[it][k]);
        }
    }
    KMC_STAMP(7);                                       // the last store is issued
#ifdef KMC_PROBE
    {
        unsigned long long st[8];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        KMC_STAMP_READ(st[0], 80, 81); KMC_STAMP_READ(st[1], 82, 83); KMC_STAMP_READ(st[2], 84, 85); KMC_STAMP_READ(st[3], 86, 87);
        KMC_STAMP_READ(st[4], 88, 89); KMC_STAMP_READ(st[5], 90, 91); KMC_STAMP_READ(st[6], 92, 93); KMC_STAMP_READ(st[7], 94, 95);
        if (lane == 0 && (tid >> 6) < 8192) for (int q = 0; q < 8; q += (KMC_PROBE == 2 ? 7 : 1)) g_probe[half][tid >> 6][q] = st[q];
    }
#endif
}

template <class Dens, int L, int K, int ITER, int SHARE>
__global__ __launch_bounds__(64 * SHARE) void half_step_vec_share(KMC_FRONT_PARAMS, const HalfStepArgs a)
{
    half_step_share_body<Dens, L, K, ITER, SHARE>(KMC_FRONT_PACK, a);
}

// Waves per workgroup of the instance that ships: two (measured at C2 against four: 3.46 against 3.55 us per burn-in half-step, the generic kernel's 3.55).
constexpr int kShareWaves = 2;

#ifdef KMC_TABLES_IMPL
// The served geometry: 32-dimensional rows with two walkers per group (L = 8, K = 2, ITER = 2: what make_plan picks from 24 576 active walkers on --
// C2's, the one geometry the instance was measured at).  SHARE <= L / ITER.
template <class D>
HalfStepFn share_part(int L, int K, int iter, int* share)
{
    *share = 0;
    if constexpr (D::kHasFrag && BlobTrait<D>::n == 0 && RowEvalTrait<D>::n == 0) {
        if (L == 8 && K == 2 && iter == 2) {
            *share = kShareWaves;
            return half_step_vec_share<D, 8, 2, 2, kShareWaves>;
        }
    }
    return nullptr;
}
#define KMC_INSTANTIATE_SHARE(D) template HalfStepFn share_part<D>(int, int, int, int*)
#endif  // KMC_TABLES_IMPL

}  // namespace kmc
