// mdl_step_halves.hpp -- the step kernel with TWO ENVS PER WAVEFRONT, one per 32-lane half, for
// the sixteen-robot configurations (A == 16, P <= 128: BASELINE config 5's 16 robots and 100
// packages): the layout's part of step_groups.  Included by mdl_step_multi.hpp (after
// mdl_step_rows.hpp, whose row helpers it uses), which holds the flow both multi-env layouts share
// and the k_step_halves entry point.
//
// Why: k_step<.., 16> runs one env per wave and is issue bound at config 5's 131,072 envs (~395
// VALU + ~264 SALU per wave at 128 waves per SIMD; profiles/r05 prices each wave instruction at ~3
// cycles per SIMD there).  Its scalar work (prologue, loop control, exec handling, ballots and
// their SALU follow-up) and every cross-lane operation serve one env.  Here env h of the wave lives
// on lanes 32h..32h+31:
//   * robot a on lanes 32h + a AND 32h + 16 + a (both 16-lane rows of the half hold every robot and
//     compute the same robot values, so a robot's data is a row-local DPP broadcast away from every
//     lane of its half, and no value has to cross the rows);
//   * package j on half-lane j & 31 of chunk j >> 5 (NC = 4 chunks, P <= 128);
//   * a minimum over the half is four in-row DPP stages plus one v_permlane16_swap (rows 0 <-> 1,
//     2 <-> 3) and a min.
// Every scalar instruction and every ballot serves both envs.  The shaped reward's nearest waiting
// package keeps k_step's compacted candidate scan, per half: each half packs its waiting candidates
// into its own LDS list and the two rows of a half scan alternate candidates for the same agent.
//
// Scope: A == 16, P <= 128 (step_halves_ok); see mdl_step_multi.hpp.
// Results are bit-identical to k_step's (tests/test_gpu_step_halves.py steps both layouts side by
// side and compares every output and the whole saved state).
#pragma once

constexpr int HALF = 32;                 // lanes per env
constexpr int HALF_NC = 4;               // package chunks per lane: P <= 128
constexpr int HALVES_MAX_P = HALF * HALF_NC;   // step_halves_ok's limit
constexpr int HALF_CAND = 136;           // candidate slots per half (<= 128 candidates, padded to a multiple of 4)

// minimum over the 32 lanes of this lane's half, on every lane of the half
__device__ __forceinline__ uint32_t half_min_u32(uint32_t m) {
    m = row_min_u32(m);
    const auto r = __builtin_amdgcn_permlane16_swap(m, m, false, false);   // [r0, r0, r2, r2], [r1, r1, r3, r3]
    return r[0] < r[1] ? r[0] : r[1];
}

// LDS bytes per wave: the carried-package gather records (4 chunks x 64 lanes x (8 + 2) B), the flag
// bytes (64 lanes x 4), the two halves' candidate lists; the reset scratch reuses the slice.
constexpr size_t HALF_GREC = (size_t)HALF_NC * 64 * 8, HALF_GPS = (size_t)HALF_NC * 64 * 2;
__host__ __device__ constexpr size_t halves_scratch_bytes() {
    return HALF_GREC + HALF_GPS + 64 * (size_t)HALF_NC + 2 * (size_t)HALF_CAND * 8;
}

// The two-envs-per-wave layout of step_groups (mdl_step_multi.hpp): group = a 32-lane half, both
// of whose 16-lane rows hold the half's 16 robots.
struct HalvesLayout {
    static constexpr int G = HALF, NC = HALF_NC;
    static constexpr uint32_t ROFF_MASK = 0x1fu;      // robot offsets h * A + ri < 32
    static constexpr uint32_t RESET_OFF_MASK = 0xffu;   // reset offsets h * P + j < 256
    static constexpr size_t FLAG_OFF = HALF_GREC + HALF_GPS;   // the flag bytes follow the gather records
    static constexpr bool RANK_BEFORE_RESET = false;
    __device__ static __forceinline__ bool stores_robot(const GroupLane q) { return (q.lane & 16) == 0; }   // row 0's copy

    // ---- the shaped reward's candidates (tracker_prev's waiting entries with st <= t): pre-step
    // state only, packed before the movement into each half's LDS list {start cell, order << 7 | slot},
    // where the order (8 bits) is a survivor's rank (< P <= 128) or 128 + slot, in the order of
    // order_key ----
    struct Near {
        int stc[NC];
        uint64_t anyw;
        uint64_t* cand;   // this lane's half's list
        int nwg;          // the (wave-uniform) padded list length
    };
    template <bool STALE>
    __device__ static __forceinline__ void near_pre(Near& nr, const GroupLane q, unsigned char* slice,
                                                    const uint32_t (&ps0)[NC], const uint64_t (&td)[NC], int t0, bool, int) {
        uint64_t wvm[NC];
        bool wv[NC];
        nr.anyw = 0;
#pragma unroll
        for (int c = 0; c < NC; c++) {
            wv[c] = !(MDL_ABLATE & 64) && trk_waiting<STALE>(ps0[c], td[c], t0);
            nr.stc[c] = pk_start(td[c]);
            wvm[c] = ballot(wv[c]);
            nr.anyw |= wvm[c];
        }
        nr.cand = (uint64_t*)(slice + HALF_GREC + HALF_GPS + 64 * NC) + q.g * HALF_CAND;
        nr.nwg = 0;
        if (nr.anyw) {
            // list position: the candidates below this lane in the whole wave (v_mbcnt), less half 0's
            // in half 1, plus the half's earlier chunks
            int n0 = 0, n1 = 0;
#pragma unroll
            for (int c = 0; c < NC; c++) {
                const int lo = popc64(wvm[c] & 0x00000000ffffffffull);
                const int below = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(wvm[c] >> 32),
                                                                 __builtin_amdgcn_mbcnt_lo((uint32_t)wvm[c], 0u));
                const int idx = below + (q.g ? n1 - lo : n0);
                const uint32_t j = (uint32_t)(c * HALF + q.gl);
                const uint32_t klo = (near_order<STALE, HALF * NC>(ps0[c], j) << 7) | j;
                if (wv[c]) nr.cand[idx] = (uint64_t)(uint32_t)nr.stc[c] | ((uint64_t)klo << 32);
                n0 += lo;
                n1 += popc64(wvm[c] & 0xffffffff00000000ull);
            }
            const int nh = q.g ? n1 : n0;
            // both halves scan the same (wave-uniform) count: each pads its list with sentinels (cell ~0:
            // no map cell, at distance >= 510 from every cell; key bits 0xffff) to a multiple of 4 of the
            // longer one
            nr.nwg = (max(n0, n1) + 3) & ~3;
            for (int k = nh + q.gl; k < nr.nwg; k += HALF) nr.cand[k] = 0x0000ffffffffffffull;
        }
    }
    // after the step: k_step's compacted candidate scan, per half
    __device__ static __forceinline__ void near_post(const Near& nr, const GroupLane q, bool, bool act, int pcell, int cell,
                                                     uint32_t& Midle, uint32_t& Mcan, int& best_cell) {
        if (nr.anyw && !(MDL_ABLATE & 32)) {
            // The two rows of a half scan alternate candidates for the same agent (two per step, two
            // LDS reads in flight): nearest key from the pre-step cell, and "a waiting package starts
            // at my new cell" (can-pick-up) into a lane mask; one swap joins the rows.  The key is one
            // v_sad_hi_u8: distance << 16 + (order << 7 | slot); a real distance is <= 508 (cells
            // are row << 8 | column, both < 255), a sentinel's >= 510.
            const uint64_t* cp = nr.cand + ((q.lane >> 4) & 1);
            uint32_t kmin = 0xffffffffu;
            uint64_t hmc = 0;
            for (int i0 = 0; i0 < nr.nwg; i0 += 4) {   // wave-uniform trip count
                const uint64_t ce = cp[i0], cf = cp[i0 + 2];
                const uint32_t ke = __builtin_amdgcn_sad_hi_u8((uint32_t)pcell, (uint32_t)ce, (uint32_t)(ce >> 32));
                const uint32_t kf = __builtin_amdgcn_sad_hi_u8((uint32_t)pcell, (uint32_t)cf, (uint32_t)(cf >> 32));
                kmin = min(kmin, min(ke, kf));
                hmc |= ballot((int)(uint32_t)ce == cell) | ballot((int)(uint32_t)cf == cell);
            }
            {
                const auto r = __builtin_amdgcn_permlane16_swap(kmin, kmin, false, false);
                kmin = r[0] < r[1] ? r[0] : r[1];
            }
            const uint32_t h16 = (uint32_t)(((hmc >> q.gbase) | (hmc >> (q.gbase + 16))) & 0xffffull);
            Mcan = ((h16 >> q.ri) & 1u) ? ~0u : 0u;
            const int js = (int)(kmin & 127u);
            const int sl = (q.gbase + (js & 31)) << 2;
            int bc = __builtin_amdgcn_ds_bpermute(sl, nr.stc[0]);
#pragma unroll
            for (int c = 1; c < NC; c++) {
                const int v = __builtin_amdgcn_ds_bpermute(sl, nr.stc[c]);
                bc = (js >> 5) == c ? v : bc;
            }
            const bool found = act && kmin < (509u << 16);
            Midle = lmask(found && (kmin >> 16) <= 3u);
            best_cell = found ? bc : -1;
        }
    }

    // ---- the pre-step carried package of each robot, through LDS: 8 bytes (env-table | tracker
    // target | deadline << 16) + 2 bytes (the pre-step state word) per package slot ----
    __device__ static __forceinline__ void gather_put(unsigned char* slice, int lane, const uint32_t (&ps0)[NC],
                                                      const uint64_t (&pk)[NC], const uint64_t (&td)[NC]) {
        uint64_t* grec = (uint64_t*)slice;
        uint16_t* gps = (uint16_t*)(slice + HALF_GREC);
#pragma unroll
        for (int c = 0; c < NC; c++) {
            grec[c * 64 + lane] = (uint64_t)tgt_dl(pk[c]) | ((uint64_t)tgt_dl(td[c]) << 32);
            gps[c * 64 + lane] = (uint16_t)ps0[c];
        }
    }
    __device__ static __forceinline__ void gather_get(unsigned char* slice, const GroupLane q, int pj, uint32_t& g_pf,
                                                      uint32_t& g_pk, uint32_t& g_td) {
        const int gi = ((pj >> 5) & (NC - 1)) * 64 + q.gbase + (pj & 31);
        const uint64_t gv = ((const uint64_t*)slice)[gi];
        g_pf = ((const uint16_t*)(slice + HALF_GREC))[gi], g_pk = (uint32_t)gv, g_td = (uint32_t)(gv >> 32);
    }

    // ---- movement partners (env.py:188-257), row-local: every row holds its half's 16 robots ----
    __device__ static __forceinline__ void partners(const GroupLane q, bool act, bool mover, uint64_t, int prop, int cell,
                                                    bool& blocked, int& occ) {
        // one word per robot: its proposal if it moves (0xffff otherwise: a non-mover blocks nobody) |
        // its cell << 16 (0xfffe where there is no robot)
        const uint32_t wd = (mover ? (uint32_t)prop : 0xffffu) | ((act ? (uint32_t)cell : 0xfffeu) << 16);
        // Each row tests its robot against half of the partners -- row 0 robots 0-7, row 1 robots
        // 8-15, fetched from row 0's copies -- and one swap joins the rows' answers.
        const int g8 = (q.lane & 16) >> 1;
        uint32_t hk = 0;
        int ok = -1;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint32_t wj = (uint32_t)__builtin_amdgcn_ds_bpermute((q.gbase + g8 + k) << 2, (int)wd);
            hk |= (wj & 0xffffu) == (uint32_t)prop ? (1u << k) : 0u;
            ok = (wj >> 16) == (uint32_t)prop ? k : ok;   // robots stand on distinct cells: one match at most
        }
        uint32_t hit = hk << g8;
        occ = ok < 0 ? -1 : ok + g8;
        {
            const auto rh = __builtin_amdgcn_permlane16_swap(hit, hit, false, false);
            hit = rh[0] | rh[1];
            const auto ro = __builtin_amdgcn_permlane16_swap((uint32_t)occ, (uint32_t)occ, false, false);
            occ = max((int)ro[0], (int)ro[1]);
        }
        // a lower-index mover into the same cell (hit holds movers only)
        blocked = (hit & ((1u << q.ri) - 1u)) != 0u;
    }

    // ---- pick-ups: per robot index J, one minimum over the half's package slots answers robot J
    // of both envs (sw: a waiting package's start cell, -2 otherwise) ----
    __device__ static __forceinline__ void pickups(const GroupLane q, unsigned char* slice, uint32_t nw, bool picker,
                                                   uint64_t pickers, const int (&sw)[NC], int cell, int& cnew) {
        constexpr uint32_t NONE = 255u;   // no package slot (slots < 128)
        if (nw & NW_SMALLMAP) {
            // Every map within 64 x 64: each half's pickers mark their cells in a 4096-bit map in LDS
            // (over the gather records, consumed before the movement); a waiting package tests one
            // bit, and the few packages under a picker are assigned in index order by the scalar
            // unit -- the first one at a picker's cell is its lowest-index package.  Cell
            // row << 8 | column is bit column & 31 of word 2 row + column / 32.
            uint32_t* pb = (uint32_t*)slice + q.g * 128;
            auto word_of = [](int cl) { return (((uint32_t)cl >> 7) | (((uint32_t)cl >> 5) & 1u)) & 127u; };
            wave_sync();
            reinterpret_cast<u32x4*>((uint32_t*)slice)[q.lane] = u32x4{0u, 0u, 0u, 0u};   // both halves' maps: 1 KB
            wave_sync();
            if (picker && stores_robot(q)) atomicOr(&pb[word_of(cell)], 1u << (cell & 31));
            wave_sync();
            uint64_t left = pickers & 0x0000ffff0000ffffull;   // row 0's robot copies
#pragma unroll
            for (int c = 0; c < NC; c++) {
                // sw < 0: some in-range word, masked (no short-circuit: no branch per chunk)
                const uint32_t bit = __builtin_amdgcn_ubfe(pb[word_of(sw[c])], (uint32_t)sw[c] & 31u, 1u);
                const uint64_t mt = ballot((sw[c] >= 0) & (bit != 0u));
                for (uint64_t m = mt; m && left; m &= m - 1) {
                    const int j = ffs64(m);
                    const uint64_t who = ballot(cell == rdl(sw[c], j)) & left & (0xffffull << (j & 32));
                    if (who) {
                        const int i = ffs64(who);
                        left &= ~(1ull << i);
                        cnew = (q.lane & ~16) == i ? c * HALF + (j & 31) + 1 : cnew;
                    }
                }
            }
        } else
        for (uint32_t u = rows_union(pickers); u; u &= u - 1) {
            const int J = __ffs((int)u) - 1;
            const int ci = __builtin_amdgcn_ds_bpermute((q.rbase + J) << 2, cell);   // robot J's cell, row-local
            uint32_t k = NONE;
#pragma unroll
            for (int c = NC - 1; c >= 0; c--) k = sw[c] == ci ? (uint32_t)(c * HALF + q.gl) : k;
            k = half_min_u32(k);
            cnew = (q.ri == J && picker && k != NONE) ? (int)k + 1 : cnew;
        }
    }

    // numpy's pairwise float32 sum of the A == 16 agents (step_halves_ok), in-row: numpy's n >= 8 form
    // r_j = x_j + x_{j+8}, ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7))
    __device__ static __forceinline__ float agent_sum(float s_lane, int) {
        const float r8 = s_lane + dppf<0x128>(s_lane);   // row_ror:8: lane j < 8 gets x_j + x_{j+8}
        const float s2 = r8 + dppf<0xB1>(r8);
        const float c4 = s2 + dppf<0x4E>(s2);
        const float d = c4 + dppf<0x124>(c4);           // lane 0: c[0] + c[12] (c[12] == c[4])
        return 0.0f + row_bcastf<0>(d);
    }

    // ---- the reset of env er2 (group base gb) by the whole wave; the half's map from its lanes'
    // registers.  *robe (store): this lane's robot word. ----
    __device__ static __forceinline__ ResetLds reset_robots(uint32_t (&)[NC], unsigned char* slice, const GroupLane q,
                                                            const DevParams& p, int P, uint32_t, int er2, int gb, int mi,
                                                            int mvoff, bool store, GLOBAL uint32_t* robe) {
        ResetLds L = reset_carve(slice, P);
        const int mr = rdl(mi, gb);
        const MapDesc md = p.maps[mr];
        const int nc = do_reset(p, er2, md, L, false);   // robot a's cell on lane a
        const int ncr = __builtin_amdgcn_ds_bpermute(q.ri << 2, nc);
        if (store) *robe = rob_pack(ncr, 0, p.movevalid_cell[(uint32_t)(mvoff + ncr)]);
        return L;
    }
};
