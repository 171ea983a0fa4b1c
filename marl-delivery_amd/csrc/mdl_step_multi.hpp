// mdl_step_multi.hpp -- the step kernels with SEVERAL ENVS PER WAVEFRONT: one flow, step_groups,
// for both layouts.  A wave is cut into groups of G lanes, one env per group:
//   k_step_rows    G = 16 (a DPP row), four envs per wave, A <= 8,  P <= 64   (mdl_step_rows.hpp)
//   k_step_halves  G = 32 (a half),    two envs per wave,  A == 16, P <= 128  (mdl_step_halves.hpp)
// Included by mdl_kernels.hip after k_step; same reference semantics (env.py:173-316,
// MAPPO/helper.py:257-369, MAPPO/trainer.py:95-130,211-259).  The two headers say why each layout
// exists and hold what differs between them (a layout struct each): the carried-package gather
// records, the nearest-waiting-package search, the movement partner match, the pick-ups, the agent
// sum, which lane copy of a robot stores, and the reset's prelude.  Everything else is here, once.
//
// Scope: full-batch steps (no env_ids), one step per launch; the one-wave-per-env k_step stays for
// everything else (subset stepping, the fused bench mode, the mailbox and step + observation
// launches, wider configs).  Results are bit-identical to k_step's (tests/test_gpu_step_rows.py and
// tests/test_gpu_step_halves.py step the layouts side by side with it).
#pragma once

// where a lane sits: env g of the wave on lanes gbase .. gbase + G - 1, package slot c * G + gl in
// chunk c, robot ri (rows: gl; halves: both 16-lane rows of a half hold every robot).  Passed to the
// layouts' functions by value: by reference, k_step_rows<1, 5, 4, *> took 6 SGPRs more and
// k_step_halves<1, 3> one VGPR (72).
struct GroupLane {
    int lane;
    int g, gl, gbase;   // lane / G, lane % G, lane - gl
    int rbase, ri;      // the lane's 16-lane DPP row: its first lane, and the lane within it
};
// the slot order inside a nearest-package key: a survivor's rank (< P <= MAXP) or MAXP + slot, as
// order_key ranks them
template <bool STALE, int MAXP>
__device__ __forceinline__ uint32_t near_order(uint32_t f, uint32_t j) {
    return STALE ? ((f & PS_SURVIVOR) ? (f >> PS_RANK_SHIFT) : (uint32_t)MAXP + j) : j;
}

#include "mdl_step_rows.hpp"
#include "mdl_step_halves.hpp"

// At reset every present entry of the group at lanes gb .. gb + G - 1 becomes a survivor ranked by its
// current key (`mine`: this lane belongs to that group); run by the whole wave.
template <bool STALE, int G, int NC>
__device__ __forceinline__ void rank_survivors(uint32_t (&ps)[NC], const GroupLane q, int P, int gb, bool mine) {
    constexpr uint64_t GMASK = ~0ull >> (64 - G);
    uint32_t rk[NC], tq[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) {
        rk[c] = 0;
        tq[c] = order_key<STALE>(ps[c], c * G + q.gl);   // the key bits survive the step's updates
    }
#pragma unroll
    for (int c2 = 0; c2 < NC; c2++) {
        uint64_t pm = ballot(c2 * G + q.gl < P && (ps[c2] & PS_PRESENT)) & (GMASK << gb);
        while (pm) {
            const uint32_t ki = (uint32_t)rdl((int)tq[c2], ffs64(pm));
            pm &= pm - 1;
#pragma unroll
            for (int c = 0; c < NC; c++) rk[c] += ki < tq[c] ? 1u : 0u;
        }
    }
#pragma unroll
    for (int c = 0; c < NC; c++) {
        if (mine) {
            if (c * G + q.gl < P && (ps[c] & PS_PRESENT)) {
                ps[c] = (ps[c] & PS_FLAGS) | PS_SURVIVOR | (rk[c] << PS_RANK_SHIFT);
            } else {
                ps[c] &= PS_STATUS;
            }
        }
    }
}

// NFULL: package chunks known to be full (slot c * G + G - 1 < P for c < NFULL): their slots need
// no "no package" handling.
template <class L, bool STALE, int NFULL>
__device__ __forceinline__ void step_groups(const uint32_t* __restrict__ rob_pre, const uint64_t* __restrict__ pkg_pre,
                                            const uint16_t* __restrict__ pst_pre, const u32x4* __restrict__ es_pre,
                                            const uint64_t* __restrict__ trk_pre, const uint8_t* __restrict__ act_pre,
                                            uint32_t ap, uint32_t nw, const StepArgs& args) {
    constexpr int G = L::G, LG = G == 16 ? 4 : 5, NC = L::NC, NG = WAVE / G, MAX_P = G * NC;
    static_assert(G == 1 << LG, "groups of 16 or 32 lanes");
    constexpr uint64_t GMASK = ~0ull >> (64 - G);   // a group's lanes, from bit 0
    static_assert(NC == 4, "one flag byte per package slot, a lane's NC slots in one 32-bit load");
    // the unclamped package loads below: element lb + c * G past the wave's first env, lb = ge * P + gl
    // masked to 8 bits -- the last group of the largest P, its last lane and chunk
    constexpr int MAX_OFF = (NG - 1) * MAX_P + (G - 1) + (NC - 1) * G;
    static_assert(MAX_OFF < PKG_PAD && MAX_OFF <= 0xff, "step_groups: package loads stay inside the buffers' padding");
    extern __shared__ __align__(16) unsigned char smem[];
    const DevParams& p = args.p;
    const StepPre pre(rob_pre, pkg_pre, pst_pre, es_pre, trk_pre, act_pre, ap, nw);
    const int A = pre.A, P = pre.P;

    const int wave = wave_id();
    const int lane = lane_id();
    const int w = pre.slot() * pre.wpb + wave;
    const int e0 = NG * w;   // this wave's envs: e0 .. e0 + NG - 1
    if (wave >= pre.wpb || e0 >= pre.n) return;
    const GroupLane q{lane, lane >> LG, lane & (G - 1), lane & (WAVE - G), lane & 48, lane & 15};
    const bool live = e0 + q.g < pre.n;   // the last wave's groups past n hold no env ...
    const int ge = live ? q.g : 0;        // ... and read env e0 (they store nothing)
    const bool act = live && q.ri < A;
    const bool rstore = L::stores_robot(q);   // this lane's copy of its robot is the one that stores

    // ---- loads: one round trip, everything independent.  No exec-masked load blocks: every lane
    // loads (lanes without data read an in-bounds word of env e0 and discard it), so the loads
    // issue back to back with no branch and no wait between them. ----
    const uint32_t roff = (uint32_t)(q.g * A + q.ri);
    // (offsets masked to their range -- g * A + ri <= ROFF_MASK, ge * P + gl < 256 -- so the loads take
    // the scalar-base + 32-bit-offset form instead of a 64-bit address per lane; slot j = c * G + gl of
    // env e0 + ge is element lb + G c, the chunks' byte offsets folded into the loads' immediates,
    // and lanes past P read the next env's slots or the 256-slot tail padding of the package
    // buffers, MdlEngine)
    const uint32_t roff_c = (act ? roff : 0u) & L::ROFF_MASK;
    const uint32_t rv_ld = (pre.rob + (size_t)e0 * A)[roff_c];
    const uint32_t ar_ld = (pre.act + (size_t)e0 * A)[roff_c];
    uint64_t pk[NC], td[NC];
    uint32_t ps[NC], ps_in[NC];
    bool dirty[NC];
    GLOBAL const uint64_t* pkge = pre.pkg + (size_t)e0 * P;
    GLOBAL const uint16_t* pste = pre.pst + (size_t)e0 * P;
    GLOBAL const uint64_t* trke = pre.trk + (size_t)e0 * P;
    bool pv[NC];   // package slot c * G + gl of this group's env exists (the stores also test live)
    const uint32_t lb = (uint32_t)(ge * P + q.gl) & 0xffu;
#pragma unroll
    for (int c = 0; c < NC; c++) {
        pv[c] = c < NFULL || c * G + q.gl < P;
        pk[c] = pkge[lb + c * G];
        ps[c] = pste[lb + c * G];
        td[c] = STALE ? trke[lb + c * G] : 0ull;
        dirty[c] = false;
    }
    // the env record's clock and total (its reward-term word is only written): two loads, so no
    // register of an unused component is recycled under a load still in flight (a forced wait)
    const uint32_t erow = (uint32_t)ge & (NG - 1);
    const uint32_t t_ld = ((GLOBAL const uint32_t*)(pre.es + e0))[4u * erow];
    const uint64_t tot_ld = ((GLOBAL const uint64_t*)(pre.es + e0))[2u * erow + 1u];
    // cost_fold[k] on group lane k (k <= A <= G): the move-cost fold of the group's n_cost movers,
    // fetched by a group-local permute once n_cost is known
    KargPtr kap = (KargPtr)((__attribute__((address_space(4))) const char*)__builtin_amdgcn_kernarg_segment_ptr() +
                            offsetof(StepKarg, args));
    const double cst = kap->p.cost_fold[q.gl];
    __builtin_amdgcn_sched_barrier(0);   // every load above is issued before any use
    const uint32_t rv = act ? rv_ld : 0u;
    int araw = act ? (int)(ar_ld & 0xffu) : 0;
    const uint32_t t_rec = t_ld;
    const uint64_t tot_rec = tot_ld;
    // Slots without a package (j >= P, or a group past n) hold sentinels that fail every test by
    // themselves, so only the loads and the stores test the slot's existence: status delivered (the
    // all-delivered test passes over them; not waiting, not present), start time 0xffff (no spawn
    // or insert while t1 < 0xffff; past that only the stores' existence test keeps them out of
    // memory), start cell 0xffff (no cell of a map of at most 255 rows).
#pragma unroll
    for (int c = 0; c < NC; c++) {
        if (c >= NFULL) {
            pk[c] = pv[c] ? pk[c] : ~0ull;
            ps[c] = pv[c] ? ps[c] : (uint32_t)ST_DELIVERED;
            td[c] = pv[c] ? td[c] : ~0ull;
        }
        ps_in[c] = ps[c];
    }
    const int fmt = args.fmt, auto_reset = args.auto_reset, lds_stride = args.lds_stride;
    const int T = p.T;
    unsigned char* slice = smem + (size_t)wave * lds_stride;
    int mvoff = p.maps[0].mvc_off;
    int mi = 0;
    if (nw & NW_MAP) {   // mixed maps: each group's map, its move-validity table by a select chain
        mi = (int)((GLOBAL const uint8_t*)p.env_map)[e0 + ge];
#pragma unroll
        for (int k = 1; k < MAX_MAPS; k++) mvoff = (mi == k) ? p.maps[k].mvc_off : mvoff;
    }
    int cell = rob_cell(rv), carry = rob_carry(rv);
    uint32_t vmask = rob_valid(rv);
    const int t0 = (int)t_rec;
    const double tot_cur = __hiloint2double((int)(uint32_t)(tot_rec >> 32), (int)(uint32_t)tot_rec);

    int mv, op;
    decode_action(araw, fmt, mv, op);
    mv = act ? mv : MV_S;
    op = act ? op : 0;
    uint32_t ps0[NC];
#pragma unroll
    for (int c = 0; c < NC; c++) {
        ps0[c] = ps[c];
        if (!STALE || !(ps0[c] & PS_SURVIVOR)) td[c] = pk[c];   // tracker_prev's view of the slot
    }

    // ---- the shaped reward's candidates (tracker_prev's waiting entries with st <= t): pre-step
    // state only, so prepared (rows: searched) before the movement ----
    typename L::Near nr;
    L::template near_pre<STALE>(nr, q, slice, ps0, td, t0, act, cell);

    // ---- the pre-step carried package of each robot, through LDS (read while the movement runs);
    // the flag bytes of the package actions (below) are cleared under the same wave barrier ----
    const int pj = carry - 1;
    unsigned char* flb = slice + L::FLAG_OFF;   // byte (group lane, c) <-> package slot c * G + gl of the group
    L::gather_put(slice, lane, ps0, pk, td);
    ((uint32_t*)flb)[lane] = 0;
    wave_sync();
    uint32_t g_pf, g_pk, g_td;   // the slot's state word, env-table and tracker target | deadline << 16
    L::gather_get(slice, q, pj, g_pf, g_pk, g_td);

    // ---- movement (env.py:188-257): every 16-lane row holds its env's robots ----
    const int pcell = cell, pcarry = carry;
    const int prop = move_proposal(act, cell, vmask, mv);
    const bool mover = !(MDL_ABLATE & 4) && act && prop != cell;
    const uint64_t movers = ballot(mover);
    const uint32_t pvm = (uint32_t)(p.movevalid_cell + mvoff)[(uint32_t)prop];
    uint64_t moved = 0;
    if (movers) {
        bool blocked;
        int occ;
        L::partners(q, act, mover, movers, prop, cell, blocked, occ);
        const uint32_t Mbase = lmask(mover && !blocked), Mfree = lmask(occ < 0);
        moved = ballot((Mbase & Mfree) != 0u);
        if (ballot((Mbase & ~Mfree) != 0u)) {   // some walk into an occupied cell: resolve the chains
            const int oln = q.rbase + (occ & 15);
            for (int it = 0; it < A; it++) {
                const uint64_t nm = ballot((Mbase & (Mfree | vbit(moved, oln))) != 0u);
                if (nm == moved) break;
                moved = nm;
            }
        }
        if ((moved >> lane) & 1ull) cell = prop;
    }
    const int n_cost = (int)__popc(row_bits(moved, q.rbase));

    // ---- package actions (env.py:259-292) ----
    // Pick-ups: each picking robot takes the lowest-index waiting package at its cell.  Robots sit on
    // distinct cells, so their choices are independent of the reference's robot order.
    const bool picker = !(MDL_ABLATE & 8) && act && op == 1 && carry == 0;
    const uint64_t pickers = ballot(picker);
    int cnew = carry;
    if (pickers) {
        int sw[NC];
#pragma unroll
        for (int c = 0; c < NC; c++) sw[c] = (ps[c] & PS_STATUS) == ST_WAITING ? pk_start(pk[c]) : -2;
        L::pickups(q, slice, nw, picker, pickers, sw, cell, cnew);
    }
    const bool picked = cnew != carry;
    carry = cnew;
    // drops: a robot with op 2 carrying a package (its pre-step one: it did not pick) and standing on
    // that package's target delivers it
    const int g_tgt = (int)(g_pk & 0xffffu), g_dl = (int)(g_pk >> 16);
    const bool drop = act && op == 2 && carry != 0 && g_tgt == cell;
    const uint64_t dmask = ballot(drop), omask = ballot(drop && t0 <= g_dl);
    // One flag byte per package slot, written by the robot concerned (each robot names at most one
    // slot, different robots different slots): picked (and now carried), delivered, carried.  The
    // package lanes read their NC slots' bytes in one word: the status changes and, for the
    // tracker update, the carried ids.
    // byte = the slot's new status (bits 0-1) | F_CHG (status changed) | F_CARRY (carried after the step)
    constexpr uint32_t F_CHG = 8u, F_CARRY = 4u;
    {
        const int fs = drop ? pj : carry - 1;
        const uint32_t fv = picked ? (F_CHG | F_CARRY | (uint32_t)ST_IN_TRANSIT)
                            : drop ? (F_CHG | (uint32_t)ST_DELIVERED) : F_CARRY;
        if (act && rstore && carry != 0) flb[(q.gbase + (fs & (G - 1))) * NC + (fs >> LG)] = (unsigned char)fv;
    }
    carry = drop ? 0 : carry;
    wave_sync();
    const uint32_t fw = ((const uint32_t*)flb)[lane];
#pragma unroll
    for (int c = 0; c < NC; c++) {   // bit arithmetic, no branch: unchanged slots' bytes have status bits 0
        const uint32_t f = fw >> (8 * c);
        const uint32_t clr = (0u - ((f >> 3) & 1u)) & PS_STATUS;
        ps[c] = (ps[c] & ~clr) | (f & PS_STATUS);
    }
    // reward: fp64 fold in the reference's order (move costs, then deliveries in robot order)
    double rr;
    {
        const int src = (q.gbase + n_cost) << 2;
        const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)__double2loint(cst));
        const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)__double2hiint(cst));
        rr = __hiloint2double((int)hi, (int)lo);
    }
    const uint32_t drow = row_bits(dmask, q.rbase), orow = row_bits(omask, q.rbase);
    if (dmask) {
        double DR = p.delivery_reward, DL = p.delay_reward;
        pin(DR);
        pin(DL);
        for (uint32_t u = rows_union(dmask); u; u &= u - 1) {
            const int i = __ffs((int)u) - 1;
            const double add = ((orow >> i) & 1u) ? DR : DL;
            rr = ((drow >> i) & 1u) ? rr + add : rr;
        }
    }
    const uint32_t rfl = (n_cost ? RT_MOVE : 0u) | (orow ? RT_ONTIME : 0u) | ((drow & ~orow) ? RT_LATE : 0u);
    const int t1 = t0 + 1;
    const double total = tot_cur + rr;

    // ---- terminate (env.py:308-316: every package delivered, or t == T) + spawn (get_state
    // env.py:133-137) ----
    uint32_t undel = 0;   // nonzero: some slot of this lane is not delivered (sentinel slots are)
    uint64_t spawned = 0;
#pragma unroll
    for (int c = 0; c < NC; c++) {
        undel |= (ps[c] & PS_STATUS) ^ (uint32_t)ST_DELIVERED;
        const bool sp = pk_st(pk[c]) == t1;
        spawned |= ballot(sp);
        ps[c] = sp ? ((ps[c] & ~PS_STATUS) | ST_WAITING) : ps[c];
    }
    // (no short-circuit: a ballot under a divergent branch costs exec juggling)
    const uint32_t alldel = lmask(((ballot(undel != 0u) >> q.gbase) & GMASK) == 0ull);
    const bool done = (lmask(live) & (lmask(t1 == T) | alldel)) != 0u;

    // ---- shaped reward with the pre-step tracker (MAPPO/helper.py:257-369) ----
    float s_lane;
    {
        const ShapeMasks<STALE> M(act, pcarry, carry, P, g_pf, pcell, cell, mv, op);
        uint32_t Midle = 0, Mcan = 0;
        int best_cell = -1;
        L::near_post(nr, q, M.need_can(), act, pcell, cell, Midle, Mcan, best_cell);
        const ShapeConsts C(p);
        s_lane = shape_terms<STALE>(M, C, (int)(g_td & 0xffffu), (int)(g_td >> 16), t1, best_cell, Midle, Mcan, pcell, cell);
    }
    const float shaped = (float)rr + L::agent_sum(s_lane, A);

    // ---- tracker update with the new state (MAPPO/trainer.py:95-130); groups that reset below
    // update with the reset state instead ----
    const bool do_rst = done && auto_reset;
    const uint64_t rst = ballot(do_rst);
    if (STALE && !(MDL_ABLATE & 2) && (ballot(picked) | dmask | spawned)) {
#pragma unroll
        for (int c = 0; c < NC; c++) {
            const bool ins = !do_rst && (pk_st(pk[c]) == t1) && !(ps[c] & PS_PRESENT);
            ps[c] = ins ? ((ps[c] & PS_STATUS) | PS_PRESENT) : ps[c];
            td[c] = ins ? pk[c] : td[c];
            dirty[c] = dirty[c] || ins;
            // present entries: carried -> in transit; in transit and not carried -> deleted (status only)
            const uint32_t m_p = lmask((ps[c] & PS_PRESENT) != 0u && !do_rst);
            const uint32_t m_c = lmask(((fw >> (8 * c)) & F_CARRY) != 0u);
            const uint32_t m_t = lmask((ps[c] & PS_TRANSIT) != 0u);
            ps[c] = (ps[c] | (PS_TRANSIT & m_c & m_p)) & (PS_STATUS | ~(m_p & ~m_c & m_t));
        }
    }

    // ---- outputs and write-back of the step (pointers fetched in one late scalar batch, as k_step).
    // A group that resets stores only its outputs and env record here: the reset below writes its
    // rows after these stores, so the package registers are dead while it runs (with the reset in the
    // middle, its path set the kernel's register count: rows 80 VGPRs and 26 SGPR spills, against 72
    // and none for the step alone; halves 85 and 28, against 72 and none) ----
    const int t_out = do_rst ? 0 : t1;
    const double total_out = do_rst ? 0.0 : total;
    vmask = (((moved >> lane) & 1ull) && !do_rst) ? pvm : vmask;
    asm volatile("" : "+v"(vmask));
    GLOBAL double* rop = (GLOBAL double*)kap->r_out;
    GLOBAL float* shp = (GLOBAL float*)kap->sh_out;
    GLOBAL uint8_t* dnp = (GLOBAL uint8_t*)kap->done_out;
    GLOBAL uint32_t* robw = (GLOBAL uint32_t*)kap->p.rob;
    GLOBAL uint16_t* pstw = (GLOBAL uint16_t*)kap->p.pstate;
    GLOBAL uint64_t* trkw = (GLOBAL uint64_t*)kap->p.trk;
    GLOBAL u32x4* esw = (GLOBAL u32x4*)kap->p.es;
    // every store: a scalar row base (env e0's) + a 32-bit lane offset, one flat predicate each
    const uint32_t er = (uint32_t)q.g & (NG - 1);
    if (live && q.gl == 0) {
        if (rop) (rop + e0)[er] = rr;
        if (shp) (shp + e0)[er] = shaped;
        if (dnp) (dnp + e0)[er] = done ? 1 : 0;
        (esw + e0)[er] = u32x4{(uint32_t)t_out, rfl, (uint32_t)__double2loint(total_out),
                               (uint32_t)__double2hiint(total_out)};
    }
    if (live && q.gl == 0 && done) {
        ((GLOBAL double*)p.ep_total + e0)[er] = total;
        ((GLOBAL int32_t*)p.ep_len + e0)[er] = t1;
    }
    if (act && rstore && !do_rst) (robw + (size_t)e0 * A)[roff] = rob_pack(cell, carry, vmask);
    const size_t eb = (size_t)e0 * P;
#pragma unroll
    for (int c = 0; c < NC; c++) {
        const uint32_t o = lb + c * G;
        // Every store tests the slot's existence (pv: j < P in a live group).  A sentinel slot's start
        // time 0xffff equals t1 once a done env steps on without reset to t = 65535, which "spawns"
        // it (and inserts it into the stale tracker); its masked offset then names the next env's
        // slot, or lies past the allocation for the last env.  (k_step guards its stores with j < P.)
        // dirty marks inserts of this step, which a resetting group does not make.
        if (live && pv[c] && !do_rst && ps[c] != ps_in[c]) (pstw + eb)[o] = (uint16_t)ps[c];
        if (STALE && live && pv[c] && dirty[c]) (trkw + eb)[o] = td[c];
    }

    // ---- reset on done (MAPPO/trainer.py:230-235): one group at a time, by the whole wave; it writes
    // the group's robots, package table and state words (and the tracker's t = 0 inserts) ----
    if (rst) {
        GLOBAL uint64_t* pkgw = (GLOBAL uint64_t*)kap->p.pkg;
        wave_sync();   // the flag bytes, gather records and candidates are consumed (the reset scratch overlays them)
        constexpr uint64_t FIRST = ~0ull / GMASK;   // every group's first lane
        for (uint64_t m = rst & FIRST; m; m &= m - 1) {
            const int gb = ffs64(m);   // the resetting group's first lane
            const int er2 = e0 + (gb >> LG);
            const bool mine = q.gbase == gb;
            if (STALE && L::RANK_BEFORE_RESET) rank_survivors<STALE, G, NC>(ps, q, P, gb, mine);
            ResetLds R = L::reset_robots(ps, slice, q, p, P, nw, er2, gb, mi, mvoff, mine && act && rstore,
                                         robw + (size_t)e0 * A + roff);
            if (STALE && !L::RANK_BEFORE_RESET) rank_survivors<STALE, G, NC>(ps, q, P, gb, mine);
#pragma unroll
            for (int c = 0; c < NC; c++) {
                const int j = c * G + q.gl;
                if (mine && j < P) {
                    const uint64_t npk = R.pk[j];
                    uint32_t nps = (uint32_t)R.pst[j] | (STALE ? (ps[c] & ~PS_STATUS) : 0u);
                    const uint32_t o = (uint32_t)(q.g * P + j) & L::RESET_OFF_MASK;
                    if (STALE) {   // the update with the reset state: inserts at t = 0, nothing carried
                        const bool ins = (pk_st(npk) == 0) & !(nps & PS_PRESENT);
                        nps = ins ? ((nps & PS_STATUS) | PS_PRESENT) : nps;
                        if (ins) (trkw + eb)[o] = npk;
                        const uint32_t upd = (nps & PS_TRANSIT) ? (nps & PS_STATUS) : nps;
                        nps = (nps & PS_PRESENT) ? upd : nps;
                    }
                    (pkgw + eb)[o] = npk;
                    (pstw + eb)[o] = (uint16_t)nps;
                }
            }
            wave_sync();   // R is read by every lane before the next group's reset rewrites it
        }
    }
}

// (rows: 93 VGPRs, 5 waves per SIMD.  Capping it at 6 waves (79 VGPRs) was 1 % faster on config 4 and
// 3-6 % slower at 4,096-16,384 envs, at 7 waves 20 % slower: profiles/r05/rows_ab.txt.)
// NFULL = 3 when P >= 48.
template <bool STALE, int AU, int NC, int NFULL>
__global__ __launch_bounds__(256) void k_step_rows(const uint32_t* __restrict__ rob_pre,
                                                   const uint64_t* __restrict__ pkg_pre,
                                                   const uint16_t* __restrict__ pst_pre,
                                                   const u32x4* __restrict__ es_pre,
                                                   const uint64_t* __restrict__ trk_pre,
                                                   const uint8_t* __restrict__ act_pre, uint32_t ap, uint32_t nw,
                                                   StepArgs args) {
    step_groups<RowsLayout<AU, NC>, STALE, NFULL>(rob_pre, pkg_pre, pst_pre, es_pre, trk_pre, act_pre, ap, nw, args);
}

// NFULL = 3 when P >= 96.
template <bool STALE, int NFULL>
__global__ __launch_bounds__(256) void k_step_halves(const uint32_t* __restrict__ rob_pre,
                                                     const uint64_t* __restrict__ pkg_pre,
                                                     const uint16_t* __restrict__ pst_pre,
                                                     const u32x4* __restrict__ es_pre,
                                                     const uint64_t* __restrict__ trk_pre,
                                                     const uint8_t* __restrict__ act_pre, uint32_t ap, uint32_t nw,
                                                     StepArgs args) {
    step_groups<HalvesLayout, STALE, NFULL>(rob_pre, pkg_pre, pst_pre, es_pre, trk_pre, act_pre, ap, nw, args);
}
