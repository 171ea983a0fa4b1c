// mdl_step_rows.hpp -- the step kernel with FOUR ENVS PER WAVEFRONT, one per 16-lane DPP row:
// the row helpers and the layout's part of step_groups (included by mdl_step_multi.hpp, which holds
// the flow both multi-env layouts share and the k_step_rows entry point).
//
// Why: at the configs' A = 5 robots and P = 50 packages, k_step's one wave per env leaves most
// lanes idle in its serial sections and pays every scalar instruction (kernel prologue, branch and
// exec-mask handling, readlane chains, loop control) once per env.  The step is issue bound at
// every measured batch (profiles/r05: ~3 cycles per wave instruction per SIMD, 4096 to 131,072
// envs).  Here env r of the wave lives on lanes 16r..16r+15: robot a on row lane a (A <= AU <= 8),
// package j on row lane j & 15 of chunk j >> 4 (NC = 4 chunks, P <= 64; an eight-chunk form for
// P <= 128 measured slower than k_step at P = 100 and was removed, profiles/r05/rows_ab.txt).  Everything an env does is
// row-local: broadcasts are DPP row_newbcast (one VALU op, no SGPR), minima are four in-row DPP
// stages, a ballot's row part is one 64-bit vector shift -- and each of those instructions serves
// four envs.  The scalar instructions are shared by the four envs as well.
//
// Scope: A <= 8, P <= 64 (step_rows_ok); see mdl_step_multi.hpp.  Results are bit-identical to
// k_step's (tests/test_gpu_step_rows.py steps both layouts side by side).
#pragma once

constexpr int ROW = 16;        // lanes per env
// package chunks per lane: NC = 4 (P <= 64), the only form built (a template parameter of the kernel)
constexpr int ROWS_MAX_P = ROW * 4;   // step_rows_ok's limit

// lane J of this lane's row, on every lane of the row (DPP row_newbcast, gfx90a+)
template <int J>
__device__ __forceinline__ int row_bcast(int v) {
    return __builtin_amdgcn_update_dpp(0, v, 0x150 + J, 0xf, 0xf, false);
}
template <int J>
__device__ __forceinline__ float row_bcastf(float v) {
    return __int_as_float(row_bcast<J>(__float_as_int(v)));
}
// this lane's row of a wave mask (bits 16r..16r+15 -> 0..15); rbase = 16r
__device__ __forceinline__ uint32_t row_bits(uint64_t m, int rbase) { return (uint32_t)(m >> rbase) & 0xffffu; }
// the union over the four rows of a wave mask
__device__ __forceinline__ uint32_t rows_union(uint64_t m) { return (uint32_t)((m | (m >> 16) | (m >> 32) | (m >> 48)) & 0xffffull); }
// minimum over the row, on every lane of the row: xor 1, xor 2, then rotations by 4 and 8
// (row_ror:n: lane l reads row lane (l - n) & 15)
__device__ __forceinline__ uint32_t row_min_u32(uint32_t m) {
    const int id = (int)0xffffffff;
    uint32_t t;
    t = (uint32_t)__builtin_amdgcn_update_dpp(id, (int)m, 0xB1, 0xf, 0xf, false); m = t < m ? t : m;   // quad_perm 1,0,3,2
    t = (uint32_t)__builtin_amdgcn_update_dpp(id, (int)m, 0x4E, 0xf, 0xf, false); m = t < m ? t : m;   // quad_perm 2,3,0,1
    t = (uint32_t)__builtin_amdgcn_update_dpp(id, (int)m, 0x124, 0xf, 0xf, false); m = t < m ? t : m;  // row_ror:4
    t = (uint32_t)__builtin_amdgcn_update_dpp(id, (int)m, 0x128, 0xf, 0xf, false); m = t < m ? t : m;  // row_ror:8
    return m;
}
__device__ __forceinline__ uint32_t row_or_u32(uint32_t m) {
    m |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0xB1, 0xf, 0xf, false);
    m |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0x4E, 0xf, 0xf, false);
    m |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0x124, 0xf, 0xf, false);
    m |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0x128, 0xf, 0xf, false);
    return m;
}

// numpy float32 add.reduce of the row's lanes 0..A-1 (A <= AU), on every lane of the row: the
// sequential n < 8 branch as a row_shr:1 chain (np_sum_lanes_dpp's argument: lanes A..AU-1 hold
// +0.0f, no lane holds -0.0f), numpy's 8-partial form when A == 8.
template <int AU>
__device__ __forceinline__ float row_np_sum(float v, int A) {
    static_assert(AU >= 1 && AU <= 8, "row_np_sum: AU <= 8");
    constexpr int L = AU < 8 ? AU : 7;
    if (AU == 8 && A == 8) {
        const float a = v + dppf<0xB1>(v);    // lanes 0, 2, 4, 6: x0+x1, x2+x3, x4+x5, x6+x7
        const float b = a + dppf<0x4E>(a);    // lanes 0, 4: (x0+x1)+(x2+x3), (x4+x5)+(x6+x7)
        const float c = b + dppf<0x124>(b);   // lane 4 (row_ror:4 reads lane l - 4): the two halves
        return 0.0f + row_bcastf<4>(c);
    }
    float t = v;
#pragma unroll
    for (int i = 1; i < L; i++) t = v + dppf<0x111>(t);   // row_shr:1 (lane 0 of the row reads +0)
    return row_bcastf<L - 1>(t);
}

// The carried package's fields a robot needs, gathered through LDS (one 16-byte record per
// package slot): its state word, env-table target | deadline << 16, tracker target | deadline << 16.
__device__ __forceinline__ uint32_t tgt_dl(uint64_t v) {
    return __builtin_amdgcn_perm((uint32_t)(v >> 32), (uint32_t)v, 0x07060302u);
}

// LDS bytes per wave: the gather records (4 chunks x 64 lanes x 16 B), then the 256 flag bytes;
// the reset scratch reuses the slice after both are consumed.
__host__ __device__ constexpr size_t rows_scratch_bytes(int NC) { return (size_t)NC * 64 * 16 + 64 * (size_t)NC; }
// where a resetting wave keeps its state words during the reset: the slice's last 512 bytes, past the
// reset scratch of P <= 64 packages (reset_lds_bytes(64) = 3,712 <= 3,840)
constexpr size_t ROWS_PS_STASH = rows_scratch_bytes(4) - 4 * 64 * 2;
static_assert(reset_lds_bytes(ROWS_MAX_P) <= ROWS_PS_STASH, "k_step_rows: the reset scratch ends before the stashed state words");

// The four-envs-per-wave layout of step_groups (mdl_step_multi.hpp): group = one DPP row.
template <int AU, int NC_>
struct RowsLayout {
    static_assert(AU >= 1 && AU <= 8, "k_step_rows: A <= 8");
    static_assert(NC_ == 4, "k_step_rows: P <= 64 (the only form built and tested)");
    static constexpr int G = ROW, NC = NC_;
    static constexpr uint32_t ROFF_MASK = 0x3fu;      // robot offsets r * A + rl < 64
    static constexpr uint32_t RESET_OFF_MASK = 0x1ffu;   // reset offsets r * P + j < 256
    static constexpr size_t FLAG_OFF = (size_t)NC * 64 * 16;   // the flag bytes follow the gather records
    // At reset the survivors are ranked first, so that the state words can wait in LDS while the
    // reset runs (registers, not LDS, bound this kernel's occupancy).
    static constexpr bool RANK_BEFORE_RESET = true;
    __device__ static __forceinline__ bool stores_robot(const GroupLane) { return true; }   // one copy per robot

    // ---- the shaped reward's pre-step part (MAPPO/helper.py:257-369): every agent's nearest waiting
    // package of tracker_prev, from its pre-step cell -- nothing here depends on this step's
    // movement or package actions, so these in-row minima are issued first and run alongside
    // those dependent chains.  Computed for all AU agents of all four rows (the terms mask
    // the agents that do not need it); key = distance << 16 + (order << 7 | slot) in one
    // v_sad_hi_u8, the order (7 bits) a survivor's rank (< P <= 64) or 64 + slot as order_key ranks
    // them (the reference's tie-break); a real distance is <= 508 (cells are row << 8 | column, both
    // < 255), a non-candidate's (cell ~0) >= 510. ----
    struct Near {
        int swv[NC];   // a candidate's start cell, -1 for none
        uint64_t anyw;
        uint32_t Midle;
        int best_cell;
    };
    template <bool STALE>
    __device__ static __forceinline__ void near_pre(Near& nr, const GroupLane q, unsigned char*, const uint32_t (&ps0)[NC],
                                                    const uint64_t (&td)[NC], int t0, bool act, int cell) {
        int stc[NC];
        uint32_t klo[NC];   // order << 7 | row-local slot, or 0xffff for no candidate
        nr.anyw = 0;
#pragma unroll
        for (int c = 0; c < NC; c++) {
            const bool wv = !(MDL_ABLATE & 64) && trk_waiting<STALE>(ps0[c], td[c], t0);
            stc[c] = pk_start(td[c]);
            nr.swv[c] = wv ? stc[c] : -1;
            const uint32_t j = (uint32_t)(c * ROW + q.gl);
            klo[c] = wv ? (near_order<STALE, ROW * NC>(ps0[c], j) << 7) | j : 0xffffu;
            nr.anyw |= ballot(wv);
        }
        nr.Midle = 0;
        nr.best_cell = -1;
        if (nr.anyw && !(MDL_ABLATE & 32)) {
            uint32_t kmin = 0xffffffffu;
#define MDL_NEAR(J)                                                                                  \
    if constexpr (J < AU) {                                                                          \
        const int pa = row_bcast<J>(cell);                                                           \
        uint32_t k = 0xffffffffu;                                                                    \
        _Pragma("unroll") for (int c = 0; c < NC; c++) {                                             \
            const uint32_t kc = __builtin_amdgcn_sad_hi_u8((uint32_t)pa, (uint32_t)nr.swv[c], klo[c]); \
            k = kc < k ? kc : k;                                                                     \
        }                                                                                            \
        k = row_min_u32(k);                                                                          \
        kmin = q.gl == J ? k : kmin;                                                                 \
    }
            MDL_NEAR(0) MDL_NEAR(1) MDL_NEAR(2) MDL_NEAR(3) MDL_NEAR(4) MDL_NEAR(5) MDL_NEAR(6) MDL_NEAR(7)
#undef MDL_NEAR
            const int js = (int)(kmin & 127u);
            const int sl = (q.gbase + (js & 15)) << 2;
            int bc = __builtin_amdgcn_ds_bpermute(sl, stc[0]);
#pragma unroll
            for (int c = 1; c < NC; c++) {
                const int v = __builtin_amdgcn_ds_bpermute(sl, stc[c]);
                bc = (js >> 4) == c ? v : bc;
            }
            const bool found = act && kmin < (509u << 16);
            nr.Midle = lmask(found && (kmin >> 16) <= 3u);
            nr.best_cell = found ? bc : -1;
        }
    }
    // after the step: the answers of near_pre, and can-pick-up (a waiting package starts at the
    // agent's new cell) for the agents that need it
    __device__ static __forceinline__ void near_post(const Near& nr, const GroupLane q, bool need_can, bool, int, int cell,
                                                     uint32_t& Midle, uint32_t& Mcan, int& best_cell) {
        Midle = nr.Midle;
        best_cell = nr.best_cell;
        if (nr.anyw && !(MDL_ABLATE & 32)) {
            if (ballot(need_can)) {
                uint32_t hm = 0;
#define MDL_CAN(J)                                                                                   \
    if constexpr (J < AU) {                                                                          \
        const int ca = row_bcast<J>(cell);                                                           \
        bool h = false;                                                                              \
        _Pragma("unroll") for (int c = 0; c < NC; c++) h = h | (nr.swv[c] == ca);                    \
        hm |= h ? (1u << J) : 0u;                                                                    \
    }
                MDL_CAN(0) MDL_CAN(1) MDL_CAN(2) MDL_CAN(3) MDL_CAN(4) MDL_CAN(5) MDL_CAN(6) MDL_CAN(7)
#undef MDL_CAN
                hm = row_or_u32(hm);
                Mcan = ((hm >> q.gl) & 1u) ? ~0u : 0u;
            }
        }
    }

    // ---- the pre-step carried package of each robot, through LDS (read while the movement runs):
    // one 16-byte record per package slot ----
    __device__ static __forceinline__ void gather_put(unsigned char* slice, int lane, const uint32_t (&ps0)[NC],
                                                      const uint64_t (&pk)[NC], const uint64_t (&td)[NC]) {
        u32x4* grec = (u32x4*)slice;
#pragma unroll
        for (int c = 0; c < NC; c++) grec[c * 64 + lane] = u32x4{ps0[c], tgt_dl(pk[c]), tgt_dl(td[c]), 0u};
    }
    __device__ static __forceinline__ void gather_get(unsigned char* slice, const GroupLane q, int pj, uint32_t& g_pf,
                                                      uint32_t& g_pk, uint32_t& g_td) {
        const u32x4 g = ((const u32x4*)slice)[((pj >> 4) & (NC - 1)) * 64 + q.gbase + (pj & 15)];
        g_pf = g.x, g_pk = g.y, g_td = g.z;
    }

    // ---- movement partners (env.py:188-257), as k_step's AU > 0 form, row-local: blocked = a
    // lower-index mover proposes the same cell; occ = the robot standing on the proposed cell ----
    __device__ static __forceinline__ void partners(const GroupLane q, bool act, bool, uint64_t movers, int prop, int cell,
                                                    bool& blocked, int& occ) {
        const int propx = act ? prop : -2, cellx = act ? cell : -3;
        int pjs[AU], cjs[AU];
#define MDL_ROWB(J)                          \
    if constexpr (J < AU) {                  \
        pjs[J] = row_bcast<J>(propx);        \
        cjs[J] = row_bcast<J>(cellx);        \
    }
        MDL_ROWB(0) MDL_ROWB(1) MDL_ROWB(2) MDL_ROWB(3) MDL_ROWB(4) MDL_ROWB(5) MDL_ROWB(6) MDL_ROWB(7)
#undef MDL_ROWB
        uint32_t hit = 0;
        occ = -1;
#pragma unroll
        for (int j = 0; j < AU; j++) {
            hit |= pjs[j] == prop ? (1u << j) : 0u;
            occ = cjs[j] == prop ? j : occ;
        }
        blocked = (hit & ((1u << q.gl) - 1u) & row_bits(movers, q.gbase)) != 0u;
    }

    // ---- pick-ups: per robot index J, one in-row minimum over the row's package slots answers
    // robot J of all four envs (sw: a waiting package's start cell, -2 otherwise) ----
    __device__ static __forceinline__ void pickups(const GroupLane q, unsigned char*, uint32_t, bool picker,
                                                   uint64_t pickers, const int (&sw)[NC], int cell, int& cnew) {
        constexpr uint32_t NONE = 255u;   // no package slot (slots < 16 * NC <= 128)
        const uint32_t pu = rows_union(pickers);
#define MDL_PICK(J)                                                                                  \
    if constexpr (J < AU) {                                                                          \
        if (pu & (1u << J)) {                                                                        \
            const int ci = row_bcast<J>(cell);                                                       \
            uint32_t k = NONE;                                                                       \
            _Pragma("unroll") for (int c = NC - 1; c >= 0; c--) k = sw[c] == ci ? (uint32_t)(c * ROW + q.gl) : k; \
            k = row_min_u32(k);                                                                      \
            cnew = (q.gl == J && picker && k != NONE) ? (int)k + 1 : cnew;                           \
        }                                                                                            \
    }
        MDL_PICK(0) MDL_PICK(1) MDL_PICK(2) MDL_PICK(3) MDL_PICK(4) MDL_PICK(5) MDL_PICK(6) MDL_PICK(7)
#undef MDL_PICK
    }

    __device__ static __forceinline__ float agent_sum(float s_lane, int A) { return row_np_sum<AU>(s_lane, A); }

    // ---- the reset of env er2 (group base gb) by the whole wave: the state words wait in LDS past
    // the reset scratch while it runs; the row's map by a scalar load (no per-lane map registers
    // live across the reset).  *robe (store): this lane's robot word. ----
    __device__ static __forceinline__ ResetLds reset_robots(uint32_t (&ps)[NC], unsigned char* slice, const GroupLane q,
                                                            const DevParams& p, int P, uint32_t nw, int er2, int, int, int,
                                                            bool store, GLOBAL uint32_t* robe) {
        uint16_t* pss = (uint16_t*)(slice + ROWS_PS_STASH);
#pragma unroll
        for (int c = 0; c < NC; c++) pss[c * 64 + q.lane] = (uint16_t)ps[c];
        ResetLds L = reset_carve(slice, P);
        const int mr = (nw & NW_MAP) ? (int)((GLOBAL const uint8_t*)p.env_map)[er2] : 0;
        const MapDesc md = p.maps[mr];
        const int nc = do_reset(p, er2, md, L, false);   // robot a's cell on lane a
        const int ncr = __builtin_amdgcn_ds_bpermute(q.ri << 2, nc);
        if (store) *robe = rob_pack(ncr, 0, p.movevalid_cell[(uint32_t)(md.mvc_off + ncr)]);
#pragma unroll
        for (int c = 0; c < NC; c++) ps[c] = pss[c * 64 + q.lane];
        return L;
    }
};
