// mdl_step_common.hpp -- the pieces of the environment step that do not depend on how envs are
// laid out on a wavefront, written once.  Included by mdl_kernels.hip before step_body; same
// reference semantics (env.py:173-316, MAPPO/helper.py:257-369, MAPPO/trainer.py:95-130).
// step_groups (the multi-env layouts, mdl_step_multi.hpp) uses all of it.  step_body (one env per
// wave) uses trk_waiting and move_proposal; it keeps its own argument unpacking, key registers and
// copy of the shaped terms, because through StepPre / order_key / ShapeMasks + shape_terms 24 of its
// instantiations took one VGPR more.
#pragma once

// The preloaded (SGPR) kernel arguments, unpacked: everything the state loads need.
struct StepPre {
    int A, P, n, wpb;
    uint32_t ap;
    GLOBAL const uint32_t* rob;
    GLOBAL const uint64_t* pkg;
    GLOBAL const uint16_t* pst;
    GLOBAL const u32x4* es;   // EnvScalars {t, ctr, total lo, total hi}
    GLOBAL const uint64_t* trk;
    GLOBAL const uint8_t* act;
    __device__ __forceinline__ StepPre(const uint32_t* rob_pre, const uint64_t* pkg_pre, const uint16_t* pst_pre,
                                       const u32x4* es_pre, const uint64_t* trk_pre, const uint8_t* act_pre,
                                       uint32_t ap, uint32_t nw)
        : A((int)(ap & 0x7fu)), P((int)((ap >> 7) & 0x7ffu)), n((int)(nw & 0xffffffu)), wpb((int)((nw >> 24) & 31u)),
          ap(ap), rob((GLOBAL const uint32_t*)rob_pre), pkg((GLOBAL const uint64_t*)pkg_pre),
          pst((GLOBAL const uint16_t*)pst_pre), es((GLOBAL const u32x4*)es_pre), trk((GLOBAL const uint64_t*)trk_pre),
          act((GLOBAL const uint8_t*)act_pre) {}
    // XCD-contiguous workgroup slots (xcd_block) from the block count packed in `ap` (a preloaded
    // SGPR: gridDim.x would cost a dispatch-packet load ahead of every state load); 0 = launch order
    __device__ __forceinline__ int slot() const {
        const int nb = (int)(ap >> AP_NB_SHIFT);
        return nb ? xcd_slot((int)blockIdx.x, nb) : (int)blockIdx.x;
    }
};

// tracker_prev's dict-order key of slot j: a survivor's rank, else ORD_EPISODE + j (stale mode)
template <bool STALE>
__device__ __forceinline__ uint32_t order_key(uint32_t f, int j) {
    return STALE ? ((f & PS_SURVIVOR) ? (f >> PS_RANK_SHIFT) : ORD_EPISODE + (uint32_t)j) : (uint32_t)j;
}
// a candidate of the shaped reward: a waiting entry of tracker_prev (state word f, data td) with st <= t0
template <bool STALE>
__device__ __forceinline__ bool trk_waiting(uint32_t f, uint64_t td, int t0) {
    const bool waiting = STALE ? ((f & PS_PRESENT) && !(f & PS_TRANSIT)) : ((f & PS_STATUS) == ST_WAITING);
    return waiting && pk_st(td) <= t0;
}

// The cell a robot proposes to move to (env.py:188-257).  Bits 1..4 of vmask only: S / other moves
// never move.  The cell delta of each move code comes from one 64-bit table of 10-bit entries
// (S 0, L -256, R +256, U -1, D +1, other 0), masked by the move's validity bit and by a vector
// mask of `act` (no exec-masked block).
__device__ __forceinline__ int move_proposal(bool act, int cell, uint32_t vmask, int mv) {
    constexpr uint64_t DTAB = (uint64_t)(0x3ffu & (uint32_t)-256) << 10 | (uint64_t)256 << 20 |
                              (uint64_t)(0x3ffu & (uint32_t)-1) << 30 | (uint64_t)1 << 40;
    const int dtab = __builtin_amdgcn_sbfe((int)(uint32_t)(DTAB >> (10 * mv)), 0, 10);
    const int vok = __builtin_amdgcn_sbfe((int)vmask, mv, 1);   // 0 or -1
    return cell + (int)(lmask(act) & (uint32_t)(dtab & vok));
}

// ---- the shaped reward (MAPPO/helper.py:257-369), agents on lanes ----
// Lane predicates as vector masks (lmask): combined on the vector ALU.  pf: the state word of the
// tracker_prev entry of the agent's previously carried id.
template <bool STALE>
struct ShapeMasks {
    uint32_t Mact, Mpc0, Mc0, Mpres, Mmov, MS, Mop1, Mop2;
    __device__ __forceinline__ ShapeMasks(bool act, int pcarry, int carry, int P, uint32_t pf, int pcell, int cell,
                                          int mv, int op) {
        Mact = lmask(act), Mpc0 = lmask(pcarry == 0), Mc0 = lmask(carry == 0);
        Mpres = Mact & ~Mpc0 & lmask(pcarry <= P) &
                (STALE ? lmask((pf & PS_PRESENT) != 0)
                       : lmask((pf & PS_STATUS) == ST_WAITING) | lmask((pf & PS_STATUS) == ST_IN_TRANSIT));
        Mmov = lmask(pcell != cell), MS = lmask(mv == MV_S);
        Mop1 = lmask(op == 1), Mop2 = lmask(op == 2);
    }
    // the agents that need the can-pick-up test
    __device__ __forceinline__ bool need_can() const { return (Mact & Mop1 & Mpc0 & Mc0) != 0u; }
};

// The reference's if-chains, term by term, as selects.  Each term is a masked constant (+0.0f when
// no branch fires; the alternatives within a term are disjoint); adding 0.0f is exact here (s
// starts at +0 and never becomes -0).  ptg / pdl: target and deadline of the tracker_prev entry of
// the previously carried id; best_cell: the nearest waiting package's start cell (-1: none); Midle:
// it is within distance 3; Mcan: a waiting package starts at the agent's new cell.  MDL_ABLATE bit 1
// (profiling builds) switches the shaping off.
// the shaping constants, pinned in SGPRs where this is constructed
struct ShapeConsts {
    float cs[9];
    __device__ __forceinline__ explicit ShapeConsts(const DevParams& p) {
#pragma unroll
        for (int k = 0; k < 9; k++) {
            cs[k] = p.shaping[k];
            pin(cs[k]);
        }
    }
};

template <bool STALE>
__device__ __forceinline__ float shape_terms(const ShapeMasks<STALE>& M, const ShapeConsts& C, int ptg, int pdl, int t1,
                                             int best_cell, uint32_t Midle, uint32_t Mcan, int pcell, int cell) {
    const float (&cs)[9] = C.cs;
    const uint32_t Mpc0 = M.Mpc0, Mc0 = M.Mc0, Mpres = M.Mpres, Mmov = M.Mmov, MS = M.MS;
    const uint32_t Mtg = lmask(cell == ptg);
    // 1. pickup / delivery
    const uint32_t Mpick = Mpc0 & ~Mc0;
    const uint32_t Mdeliv = ~Mpc0 & Mc0 & Mpres & Mtg;
    const float t1v = fmask(Mpick, cs[SH_PICK]) + fmask(Mdeliv, fpick(lmask(t1 <= pdl), cs[SH_ONTIME], cs[SH_LATE]));
    // 2. wasted operations
    const uint32_t Mwpick = M.Mop1 & (~Mpc0 | (Mc0 & ~Mcan));
    const uint32_t Mwdrop = M.Mop2 & (Mpc0 | (~Mc0 & Mpres & ~Mtg));
    const float t2v = fmask(Mwpick, cs[SH_WPICK]) + fmask(Mwdrop, cs[SH_WDROP]);
    // 3. movement
    const float t3v = fmask(~MS & ~Mmov, cs[SH_STUCK]);
    const int tgt = ipick(~Mpc0 & Mpres, ptg, best_cell);
    const int db = manhattan_sad(pcell, tgt), da = manhattan_sad(cell, tgt);   // garbage for tgt < 0: masked
    const uint32_t Mt = lmask(tgt >= 0) & Mmov;
    const float t4v = fmask(Mt & lmask(da < db), cs[SH_CLOSER]) + fmask(Mt & lmask(da > db), cs[SH_AWAY]);
    // 4. idle next to an available package
    const float t5v = fmask(~Mmov & MS & Mpc0 & Midle, cs[SH_IDLE]);
    // (0.0f + t1v == t1v: t1v is a sum of two terms of which one is +0, so never -0)
    float s = t1v;
    s = s + t2v;
    s = s + t3v;
    s = s + t4v;
    s = s + t5v;
    return fmask((MDL_ABLATE & 1) ? 0u : M.Mact, s);
}
