// mdl_alt_ego.hpp -- robot-centred windows of the IDQ / map-QMIX agent observation
// (mdl_build_obs_alt_ego, k_alt_ego).
//
// For radius R (1..15, K = 2R + 1) robot a on cell (r, c) gets the K x K crop of its convert_state
// tensor (IDQ/networks.py:112-217 == qmix/networks.py:243-348, what k_alt_obs writes) centred on itself:
//   ego[a][ch][i][j] = idq_obs[a][ch][r - R + i][c - R + j]   inside the map,
//   1.0 in channel 0 and 0.0 in channels 1-5 outside it.
// float32 only: channel 1 holds the urgency floats, which a half type would round, and the replay
// rings append float rows.  The output shape [A][6][K][K] does not depend on the map, so one launch may
// cross map shapes: every wave reads its own env's MapDesc.
//
// One wave per env.  LDS per wave (alt_ego_lds_bytes):
//   tracker slots   obs_pre_bytes(P)          (stage_tracker, as the other builders)
//   rcell, rtgt     int32[A] each             robot a's packed cell | carrying << 16; its carried id's
//                                             target cell when the id is in the tracker, else -1
//   bits            uint32[3][NW]             obstacles, robots, waiting-start cells (AE_*)
//   urg             float[HW]                 alt_prepare's per-cell urgency; 0 where no package waits
//   image           uint32[ego_image_words]   flat bit image of a group of robots' windows
// which is k_alt_obs's slice less its three byte planes and three of its six bitsets, plus the robot
// words (8 B each, against 3 B per cell there) and one image.
//
// The five 0/1 channels and the support of channel 1 (the waiting-start bits; channels 1 and 2 are
// zero for a carrying robot) are K-bit fields packed in output order, as mdl_ego.hpp's image.  The
// emitter turns bits into floats; where a float4 group overlaps a channel-1 block and has a bit set,
// each such 1.0 is replaced by the urgency of the map cell under that window cell.
//
// No window coordinate indexes LDS or global memory unclamped: rows outside [0, H) are constants, the
// word index of a funnel shift is clamped to [0, NW) (ego_bits32) and the bits of columns outside
// [0, W) are masked, so a set bit of channel 1 is a set start bit of a cell inside the map and the
// urgency read at that cell (clamped to [0, HW) all the same) stays inside urg.  Image reads are by
// element index < the group's element count, plus the one word ego_image_words adds.  Every output
// element is written once: the dword head, the float4 body and the dword tail of a group partition it.
//
// Included by mdl_kernels.hip, inside namespace mdl, after mdl_ego.hpp (ego_bits32, ego_image_words,
// EGO_IMAGE_BYTES).
#pragma once

enum : int { AE_GRID = 0, AE_ROB, AE_START, AE_NBS };

__host__ __device__ inline size_t alt_ego_fixed_bytes(int A, int P, int HW) {
    return obs_pre_bytes(P) + 2 * align16(sizeof(int32_t) * (size_t)A) +
           align16(sizeof(uint32_t) * AE_NBS * (size_t)((HW + 31) / 32)) + align16(sizeof(float) * (size_t)HW);
}
__host__ __device__ inline size_t alt_ego_lds_bytes(int A, int P, int HW, int G, int K) {
    return alt_ego_fixed_bytes(A, P, HW) + align16(sizeof(uint32_t) * (size_t)ego_image_words(G, K));
}

struct AltEgoLds {
    int32_t *rcell, *rtgt;
    uint32_t* bits;   // [AE_NBS][NW]
    float* urg;       // [HW]
    uint32_t* img;
};

__device__ inline AltEgoLds alt_ego_carve(unsigned char* base, int A, int HW) {
    AltEgoLds L;
    const int NW = (HW + 31) >> 5;
    size_t o = 0;
    L.rcell = (int32_t*)(base + o); o += align16(sizeof(int32_t) * (size_t)A);
    L.rtgt = (int32_t*)(base + o); o += align16(sizeof(int32_t) * (size_t)A);
    L.bits = (uint32_t*)(base + o); o += align16(sizeof(uint32_t) * AE_NBS * (size_t)NW);
    L.urg = (float*)(base + o); o += align16(sizeof(float) * (size_t)HW);
    L.img = (uint32_t*)(base + o);
    return L;
}

// What the windows read of alt_prepare: the robots, the three bitsets and the urgency floats (the same
// alt_urgency values under the same max rule; 0 bits where alt_prepare keeps -1, the start bit telling
// the two apart).  Robots come in on lanes (lane a < A): cell packed r | c << 8, carry id.
template <class Trk>
__device__ __forceinline__ void alt_ego_prepare(const Trk& trk, const AltEgoLds& L, const uint32_t* gridbits, int HW,
                                                int W, int A, int t, int cell, int carry) {
    const int lane = lane_id();
    const int NW = (HW + 31) >> 5;
    if (lane < A) {
        L.rcell[lane] = cell | (carry != 0 ? 1 << 16 : 0);
        const int cs = carry != 0 ? trk.slot_of(carry) : -1;
        L.rtgt[lane] = cs >= 0 ? pk_target(trk.data(cs)) : -1;   // no in-transit condition (alt_emit_fast)
    }
    for (int w = lane; w < NW; w += WAVE) {
        L.bits[AE_GRID * NW + w] = gridbits[w];
        L.bits[AE_ROB * NW + w] = 0;
        L.bits[AE_START * NW + w] = 0;
    }
    float4* u4 = reinterpret_cast<float4*>(L.urg);   // align16(4 * HW) bytes: whole float4s
    for (int i = lane; i < (HW + 3) >> 2; i += WAVE) u4[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    wave_sync();
    if (lane < A) {
        const unsigned rc = (unsigned)(cell_r(cell) * W + cell_c(cell));
        if (rc < (unsigned)HW) atomicOr(&L.bits[AE_ROB * NW + (rc >> 5)], 1u << (rc & 31));
    }
    for (int j = lane; j < trk.count(); j += WAVE) {
        if (!trk.present(j) || trk.in_transit(j)) continue;
        const uint64_t d = trk.data(j);
        const int st = pk_st(d);
        if (!(t >= st)) continue;
        const int sc = pk_start(d);
        const unsigned si = (unsigned)(cell_r(sc) * W + cell_c(sc));
        if (si < (unsigned)HW) {
            // urgencies are >= 0, so their float bits order like ints
            atomicMax((int*)&L.urg[si], __float_as_int(alt_urgency(t, st, pk_dl(d))));
            atomicOr(&L.bits[AE_START * NW + (si >> 5)], 1u << (si & 31));
        }
    }
    wave_sync();
}

// Window row i of (robot a, channel ch) as a K-bit field: bit j is column c - R + j of map row
// r - R + i.  Bits K..31 are zero.  Channel 1's field is its support, the waiting-start bits.
__device__ __forceinline__ uint32_t alt_ego_field(const AltEgoLds& L, int NW, int H, int W, int R, int a, int ch,
                                                  int i) {
    const int K = 2 * R + 1;
    const uint32_t km = (1u << K) - 1u;   // K <= 31
    const uint32_t own = i == R ? 1u << R : 0u;
    if (ch == 4) return own;
    const int rc = L.rcell[a];
    const int rr = cell_r(rc) - R + i, c0 = cell_c(rc) - R;
    if ((unsigned)rr >= (unsigned)H) return ch == 0 ? km : 0u;   // a row above or below the map
    if ((ch == 1 || ch == 2) && (rc >> 16)) return 0u;            // a carrying robot sees no waiting package
    if (ch == 5) {   // one-hot of the carried id's target, where the window holds it
        const int tg = L.rtgt[a];
        const unsigned d = (unsigned)(cell_c(tg) - c0);
        return (tg >= 0 && cell_r(tg) == rr && d < (unsigned)K) ? 1u << d : 0u;
    }
    // columns inside the map: j in [lo, hi), never empty (j = R is the robot's own column)
    const int lo = c0 < 0 ? -c0 : 0, hi = min(K, W - c0);
    const uint32_t cm = ((1u << hi) - 1u) & ~((1u << lo) - 1u);
    // the row's bits from its first in-map column, moved up to that column's place in the field
    const int b = rr * W + (c0 < 0 ? 0 : c0);
    if (ch == 0) return ((ego_bits32(L.bits + AE_GRID * NW, NW, b) << lo) & cm) | (km & ~cm);
    if (ch == 3) return (ego_bits32(L.bits + AE_ROB * NW, NW, b) << lo) & cm & ~own;   // the other robots
    return (ego_bits32(L.bits + AE_START * NW, NW, b) << lo) & cm;
}

// The windows of robots [a0, a0 + na) as a flat bit image (ego_build_image's packing on this
// featurizer's fields): lane k builds word k from the fields that overlap it.
__device__ __forceinline__ void alt_ego_build_image(const AltEgoLds& L, int NW, int H, int W, int R, int a0, int na) {
    const int lane = lane_id();
    const int K = 2 * R + 1, nrow = na * 6 * K, nfw = (nrow * K + 31) >> 5;
    const float inv_k = 1.0f / (float)K;
    for (int k = lane; k < nfw; k += WAVE) {
        const int g0 = k << 5;   // < 2^23: fdivi is exact
        int p = fdivi(g0, K, inv_k);
        int c0 = g0 - p * K;
        const int pl = fdivi(p, K, inv_k);
        int i = p - pl * K;
        int al = pl / 6, ch = pl - 6 * al;
        uint32_t out = 0;
        int pos = 0;
        while (pos < 32 && p < nrow) {
            out |= (alt_ego_field(L, NW, H, W, R, a0 + al, ch, i) >> c0) << pos;
            pos += K - c0;
            c0 = 0;
            p++;
            if (++i == K) {
                i = 0;
                if (++ch == 6) {
                    ch = 0;
                    al++;
                }
            }
        }
        L.img[k] = out;
    }
    if (lane == 0) L.img[nfw] = 0u;   // the word the emitter reads after the last
    wave_sync();
}

// n = na * 6 * K * K floats of the image of robots [a0, a0 + na) at dst (any 4-byte alignment): a dword
// head to 16-B alignment, a float4 body whose 4-bit groups start at bit head + 4q (a group may straddle
// two words: the word after its first is read with it) and a dword tail.  A set bit is 1.0, except in
// a channel-1 block, where it is the urgency of the map cell under it.  The body tells by the group's
// offset within its robot (rem, kept by addition) whether it overlaps channel 1 at all.
__device__ __forceinline__ void alt_ego_emit(const AltEgoLds& L, int HW, int W, int R, int a0, int n, float* dst) {
    const int lane = lane_id();
    const int K = 2 * R + 1, KK = K * K, per = 6 * KK;
    const float inv_k = 1.0f / (float)K, inv_per = 1.0f / (float)per;
    const uint32_t* FB = L.img;
    // element idx < n (< 2^23) whose bit is set
    auto set_value = [&](int idx) -> float {
        const int al = fdivi(idx, per, inv_per);
        const int q = idx - al * per - KK;
        if ((unsigned)q >= (unsigned)KK) return 1.0f;
        const int i = fdivi(q, K, inv_k), j = q - i * K;
        const int rc = L.rcell[a0 + al];
        const int m = (cell_r(rc) - R + i) * W + cell_c(rc) - R + j;   // inside the map: its start bit is set
        return L.urg[min(max(m, 0), HW - 1)];
    };
    // head and tail: at most 3 elements at either end of whole robots' windows, so of a channel 0 or 5
    auto one = [&](int idx) -> float { return ((FB[idx >> 5] >> (idx & 31)) & 1u) ? 1.0f : 0.0f; };
    int head = (int)(((16 - ((uintptr_t)dst & 15)) & 15) >> 2);
    if (head > n) head = n;
    if (lane < head) dst[lane] = one(lane);
    const int nb = (n - head) >> 2;
    float4* d4 = reinterpret_cast<float4*>(dst + head);
    int i0 = head + 4 * lane;                       // <= 255
    int rem = i0 - fdivi(i0, per, inv_per) * per;   // i0 mod per
    const int step = 4 * WAVE - fdivi(4 * WAVE, per, inv_per) * per;
    for (int q = lane; q < nb; q += WAVE) {
        const uint32_t* w = FB + (i0 >> 5);
        const uint32_t nib = __builtin_amdgcn_alignbit(w[1], w[0], (uint32_t)(i0 & 31)) & 15u;
        float4 v = float4_of_bits(nib);
        if (nib != 0u && rem + 3 >= KK && rem < 2 * KK) {   // rare: a waiting package in a channel-1 block
            if (nib & 1u) v.x = set_value(i0);
            if (nib & 2u) v.y = set_value(i0 + 1);
            if (nib & 4u) v.z = set_value(i0 + 2);
            if (nib & 8u) v.w = set_value(i0 + 3);
        }
        d4[q] = v;
        i0 += 4 * WAVE;
        rem += step;
        if (rem >= per) rem -= per;
    }
    const int tail = head + 4 * nb;
    if (tail + lane < n) dst[tail + lane] = one(tail + lane);
}

// idq_ego [n][A][6][K][K] of envs [env_begin, env_begin + n), K = 2R + 1; G robots per image (the
// host's alt_ego_group).  rows: null, or uint8 [E] indexed by env id, non-zero = build.  The wave of an
// unmarked env leaves after that one byte load, before it touches LDS, and writes nothing; the kernel
// has no workgroup barrier, so a whole wave may return.
template <bool STALE>
__global__ __launch_bounds__(256) void k_alt_ego(DevParams p, int env_begin, int n, int R, float* __restrict__ out,
                                                 int wpb, int lds_stride, int G, const uint8_t* __restrict__ rows) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int wave = wave_id();
    const int lane = lane_id();
    const int w = xcd_block() * wpb + wave;
    if (wave >= wpb || w >= n) return;
    const int e = env_begin + w;
    if (rows && __builtin_amdgcn_readfirstlane((int)rows[e]) == 0) return;   // wave-uniform, before any LDS use
    const int A = p.A, P = p.P;
    unsigned char* base = smem + (size_t)wave * lds_stride;
    ObsLdsPre S = obs_pre_carve(base, P);
    const MapDesc md = p.maps[p.env_map ? p.env_map[e] : 0];
    const int H = md.H, W = md.W, HW = H * W, NW = (HW + 31) >> 5;
    const AltEgoLds L = alt_ego_carve(base + obs_pre_bytes(P), A, HW);
    const int t = p.es[e].t;
    const uint32_t rv = lane < A ? p.rob[(size_t)e * A + lane] : 0u;
    stage_tracker<STALE>(p, e, P, lane, S);
    alt_ego_prepare(staged_tracker<STALE>(S, P), L, p.gridbits + md.bits_off, HW, W, A, t, rob_cell(rv), rob_carry(rv));
    const int per = 6 * (2 * R + 1) * (2 * R + 1);   // elements per robot
    float* dst = out + (size_t)w * A * per;
    for (int a0 = 0; a0 < A; a0 += G) {   // uniform
        const int na = min(G, A - a0);
        alt_ego_build_image(L, NW, H, W, R, a0, na);
        alt_ego_emit(L, HW, W, R, a0, na * per, dst + (size_t)a0 * per);
        wave_sync();   // the image is rebuilt for the next group
    }
}
