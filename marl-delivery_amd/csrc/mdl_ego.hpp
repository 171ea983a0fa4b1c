// mdl_ego.hpp -- robot-centred actor-map windows (mdl_build_obs_ego, k_ego_maps).
//
// For radius R (1..15, K = 2R + 1) robot a on cell (r, c) gets the K x K crop of its
// convert_observation tensor (MAPPO/helper.py:6-66) centred on itself:
//   ego[a][ch][i][j] = full[a][ch][r - R + i][c - R + j]   inside the map,
//   1.0 in channel 0 (an off-map cell cannot be entered) and 0.0 in channels 1-5 outside it.
// The output shape [A][6][K][K] does not depend on the map, so one launch may cross map shapes:
// every wave reads its own env's MapDesc.
//
// One wave per env.  LDS per wave (ego_lds_bytes):
//   tracker slots   obs_pre_bytes(P)         (stage_tracker, as the other builders)
//   rcell, rtgt     int32[64] each           robot a's packed cell, its carried target's (or -1)
//   bits            uint32[5][NW]            the cell bitsets of feat_prepare (BS_*)
//   image           uint32[ego_image_words]  flat bit image of a group of robots' windows
// Every (robot, channel, window row) is one K-bit field: a funnel shift of two bitset words at the
// row's first in-map cell, masked to the columns inside the map.  The fields are packed back to back
// (bit ((a * 6 + ch) * K + i) * K + j: element order of the output) and streamed by the flat emitters.
// No window coordinate indexes LDS unclamped: rows outside [0, H) are constants, the word index of a
// funnel shift is clamped to [0, NW) and the bits of columns outside [0, W) are masked.
//
// Included by mdl_kernels.hip, inside namespace mdl, after the tracker staging (ObsLdsPre,
// stage_tracker) and the builders' headers (mdl_features.hpp, mdl_obs_small.hpp).
#pragma once

constexpr int EGO_RMAX = 15;            // K = 31: a window row within one 32-bit word
constexpr int EGO_IMAGE_BYTES = 8192;   // the image of one robot group (A = 64, R = 15 is 46 KB in all)

// words of the image of G robots' windows: the bits, and one word more (the emitters' funnel shifts
// read the word after a group's first)
__host__ __device__ inline int ego_image_words(int G, int K) { return (G * 6 * K * K + 31) / 32 + 1; }

__host__ __device__ inline size_t ego_fixed_bytes(int P, int HW) {
    return obs_pre_bytes(P) + align16(sizeof(int32_t) * 64 * 2) + align16(sizeof(uint32_t) * 5 * (size_t)((HW + 31) / 32));
}
__host__ __device__ inline size_t ego_lds_bytes(int P, int HW, int G, int K) {
    return ego_fixed_bytes(P, HW) + align16(sizeof(uint32_t) * (size_t)ego_image_words(G, K));
}

struct EgoLds {
    int32_t *rcell, *rtgt;
    uint32_t* bits;   // [5][NW]
    uint32_t* img;
};

__device__ inline EgoLds ego_carve(unsigned char* base, int NW) {
    EgoLds L;
    L.rcell = (int32_t*)base;
    L.rtgt = L.rcell + 64;
    size_t o = align16(sizeof(int32_t) * 64 * 2);
    L.bits = (uint32_t*)(base + o); o += align16(sizeof(uint32_t) * 5 * (size_t)NW);
    L.img = (uint32_t*)(base + o);
    return L;
}

// feat_prepare's robots and cell bitsets, without the sorts, carriers and critic order the windows do
// not need.  Robots come in on lanes (lane a < A): cell packed r | c << 8, carry id.
template <class Trk>
__device__ __forceinline__ void ego_prepare(const Trk& trk, const EgoLds& L, const uint32_t* gridbits, int NW, int W,
                                            int A, int NS, int t, int cell, int carry) {
    const int lane = lane_id();
    const unsigned nbits = (unsigned)NW << 5;
    if (lane < A) {
        L.rcell[lane] = cell;
        const int cs = carry != 0 ? trk.slot_of(carry) : -1;
        int tg = -1;
        if (cs >= 0 && trk.in_transit(cs)) tg = pk_target(trk.data(cs));
        L.rtgt[lane] = tg;   // convert_observation channel 5 (MAPPO/helper.py:59-64)
    }
    for (int w = lane; w < NW; w += WAVE) {
        L.bits[BS_GRID * NW + w] = gridbits[w];
        L.bits[BS_ROBOT * NW + w] = 0;
        L.bits[BS_MULTI * NW + w] = 0;
        L.bits[BS_WSTART * NW + w] = 0;
        L.bits[BS_ATARGET * NW + w] = 0;
    }
    wave_sync();
    if (lane < A) {
        const unsigned rc = (unsigned)(cell_r(cell) * W + cell_c(cell));
        if (rc < nbits) {
            const uint32_t m = 1u << (rc & 31);
            const uint32_t old = atomicOr(&L.bits[BS_ROBOT * NW + (rc >> 5)], m);
            if (old & m) atomicOr(&L.bits[BS_MULTI * NW + (rc >> 5)], m);   // a second robot on the cell
        }
    }
    for (int j0 = 0; j0 < NS; j0 += WAVE) {
        const int j = j0 + lane;
        if (j < NS && trk.present(j)) {
            const uint64_t d = trk.data(j);
            const bool it = trk.in_transit(j);
            const bool wt = !it && pk_st(d) <= t;
            const int tg = pk_target(d), sc = pk_start(d);
            if (wt) {
                const unsigned ci = (unsigned)(cell_r(sc) * W + cell_c(sc));
                if (ci < nbits) atomicOr(&L.bits[BS_WSTART * NW + (ci >> 5)], 1u << (ci & 31));
            }
            if (wt || it) {
                const unsigned ci = (unsigned)(cell_r(tg) * W + cell_c(tg));
                if (ci < nbits) atomicOr(&L.bits[BS_ATARGET * NW + (ci >> 5)], 1u << (ci & 31));
            }
        }
    }
    wave_sync();
}

// The 32 bits of a bitset (NW words) from bit b on.  Both word indices are clamped to [0, NW): bits
// read through a clamped index belong to cells past the map row asked for, which the caller masks.
__device__ __forceinline__ uint32_t ego_bits32(const uint32_t* bs, int NW, int b) {
    const int w0 = min(max(b >> 5, 0), NW - 1), w1 = min(w0 + 1, NW - 1);
    return __builtin_amdgcn_alignbit(bs[w1], bs[w0], (uint32_t)(b & 31));
}

// Window row i of (robot a, channel ch) as a K-bit field: bit j is column c - R + j of map row
// r - R + i.  Bits K..31 are zero.
__device__ __forceinline__ uint32_t ego_field(const EgoLds& L, int NW, int H, int W, int R, int a, int ch, int i) {
    const int K = 2 * R + 1;
    const uint32_t km = (1u << K) - 1u;   // K <= 31
    const uint32_t own = i == R ? 1u << R : 0u;
    if (ch == 1) return own;
    const int cell = L.rcell[a];
    const int rr = cell_r(cell) - R + i, c0 = cell_c(cell) - R;
    if ((unsigned)rr >= (unsigned)H) return ch == 0 ? km : 0u;   // a row above or below the map
    // columns inside the map: j in [lo, hi), never empty (j = R is the robot's own column)
    const int lo = c0 < 0 ? -c0 : 0, hi = min(K, W - c0);
    const uint32_t cm = ((1u << hi) - 1u) & ~((1u << lo) - 1u);
    if (ch == 5) {   // one-hot of the carried package's target, where the window holds it
        const int tg = L.rtgt[a];
        const unsigned d = (unsigned)(cell_c(tg) - c0);
        return (tg >= 0 && cell_r(tg) == rr && d < (unsigned)K) ? 1u << d : 0u;
    }
    // the row's bits from its first in-map column, moved up to that column's place in the field
    const int b = rr * W + (c0 < 0 ? 0 : c0);
    if (ch == 0) return ((ego_bits32(L.bits + BS_GRID * NW, NW, b) << lo) & cm) | (km & ~cm);
    if (ch == 2)
        return (((ego_bits32(L.bits + BS_ROBOT * NW, NW, b) << lo) & ~own) |
                (ego_bits32(L.bits + BS_MULTI * NW, NW, b) << lo)) & cm;
    return (ego_bits32(L.bits + (ch == 3 ? BS_WSTART : BS_ATARGET) * NW, NW, b) << lo) & cm;
}

// The windows of robots [a0, a0 + na) as a flat bit image (build_flat's packing with K-bit rows):
// lane k builds word k from the fields that overlap it, walking (robot, channel, row) in step.
__device__ __forceinline__ void ego_build_image(const EgoLds& L, int NW, int H, int W, int R, int a0, int na) {
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
            out |= (ego_field(L, NW, H, W, R, a0 + al, ch, i) >> c0) << pos;
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
    if (lane == 0) L.img[nfw] = 0u;   // the word the emitters read after the last
    wave_sync();
}

// n floats of a flat bit image at dst, any 4-byte alignment: emit_flat4 for a 16-B aligned dst, else
// a dword head to 16-B alignment, a float4 body whose 4-bit groups start at bit head + 4q (a group
// may straddle two words: the word after its first is read with it) and a dword tail.
__device__ __forceinline__ void ego_emit(const uint32_t* FB, int n, float* dst) {
    if (((uintptr_t)dst & 15) == 0) {
        emit_flat4(FB, n, dst);
        return;
    }
    const int lane = lane_id();
    auto one = [&](int i) -> float { return ((FB[i >> 5] >> (i & 31)) & 1u) ? 1.0f : 0.0f; };
    int head = (int)(((16 - ((uintptr_t)dst & 15)) & 15) >> 2);
    if (head > n) head = n;
    if (lane < head) dst[lane] = one(lane);
    const int nb = (n - head) >> 2;
    float4* d4 = reinterpret_cast<float4*>(dst + head);
    for (int q = lane; q < nb; q += WAVE) {
        const int i0 = head + 4 * q;
        const uint32_t* w = FB + (i0 >> 5);
        d4[q] = float4_of_bits(__builtin_amdgcn_alignbit(w[1], w[0], (uint32_t)(i0 & 31)) & 15u);
    }
    const int tail = head + 4 * nb;
    if (tail + lane < n) dst[tail + lane] = one(tail + lane);
}
template <class OT>
__device__ __forceinline__ void ego_emit(const uint32_t* FB, int n, OT* dst) {
    emit_flat_h(FB, n, dst);
}

// out [n][A][6][K][K] of envs [env_begin, env_begin + n), K = 2R + 1; G robots per image (the host's
// ego_group: the whole env where its image fits the slice).  k_masked_ego_maps below repeats this body
// behind a row mask: a change to one belongs in the other.
template <bool STALE, class OT>
__global__ __launch_bounds__(256) void k_ego_maps(DevParams p, int env_begin, int n, int R, OT* __restrict__ out,
                                                  int wpb, int lds_stride, int G) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int wave = wave_id();
    const int lane = lane_id();
    const int w = xcd_block() * wpb + wave;
    if (wave >= wpb || w >= n) return;
    const int e = env_begin + w;
    const int A = p.A, P = p.P;
    unsigned char* base = smem + (size_t)wave * lds_stride;
    ObsLdsPre S = obs_pre_carve(base, P);
    const MapDesc md = p.maps[p.env_map ? p.env_map[e] : 0];
    const int H = md.H, W = md.W, NW = (H * W + 31) >> 5;
    const EgoLds L = ego_carve(base + obs_pre_bytes(P), NW);
    const int t = p.es[e].t;
    const uint32_t rv = lane < A ? p.rob[(size_t)e * A + lane] : 0u;
    stage_tracker<STALE>(p, e, P, lane, S);
    ego_prepare(staged_tracker<STALE>(S, P), L, p.gridbits + md.bits_off, NW, W, A, P, t, rob_cell(rv), rob_carry(rv));
    const int per = 6 * (2 * R + 1) * (2 * R + 1);   // elements per robot
    OT* dst = out + (size_t)w * A * per;
    for (int a0 = 0; a0 < A; a0 += G) {   // uniform
        const int na = min(G, A - a0);
        ego_build_image(L, NW, H, W, R, a0, na);
        [[clang::always_inline]] ego_emit(L.img, na * per, dst + (size_t)a0 * per);
        wave_sync();   // the image is rebuilt for the next group
    }
}

// k_ego_maps under a row mask (mdl_build_obs_ego_masked), on the same device functions: rows (uint8 [E],
// indexed by env id, non-zero = build) marks the envs to build.  The wave of an unmarked env leaves after
// one byte load, before it touches LDS, and writes nothing; the kernel has no workgroup barrier, so a
// whole wave may return.  Launch shape, slices and output rows (env e = env_begin + w at
// out + w * A * 6 * K * K) are k_ego_maps's.  A sibling, not a template flag: k_ego_maps keeps its code.
template <bool STALE, class OT>
__global__ __launch_bounds__(256) void k_masked_ego_maps(DevParams p, int env_begin, int n, int R,
                                                         OT* __restrict__ out, int wpb, int lds_stride, int G,
                                                         const uint8_t* __restrict__ rows) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int wave = wave_id();
    const int lane = lane_id();
    const int w = xcd_block() * wpb + wave;
    if (wave >= wpb || w >= n) return;
    const int e = env_begin + w;
    if (__builtin_amdgcn_readfirstlane((int)rows[e]) == 0) return;   // wave-uniform: one byte, before any LDS use
    const int A = p.A, P = p.P;
    unsigned char* base = smem + (size_t)wave * lds_stride;
    ObsLdsPre S = obs_pre_carve(base, P);
    const MapDesc md = p.maps[p.env_map ? p.env_map[e] : 0];
    const int H = md.H, W = md.W, NW = (H * W + 31) >> 5;
    const EgoLds L = ego_carve(base + obs_pre_bytes(P), NW);
    const int t = p.es[e].t;
    const uint32_t rv = lane < A ? p.rob[(size_t)e * A + lane] : 0u;
    stage_tracker<STALE>(p, e, P, lane, S);
    ego_prepare(staged_tracker<STALE>(S, P), L, p.gridbits + md.bits_off, NW, W, A, P, t, rob_cell(rv), rob_carry(rv));
    const int per = 6 * (2 * R + 1) * (2 * R + 1);   // elements per robot
    OT* dst = out + (size_t)w * A * per;
    for (int a0 = 0; a0 < A; a0 += G) {   // uniform
        const int na = min(G, A - a0);
        ego_build_image(L, NW, H, W, R, a0, na);
        [[clang::always_inline]] ego_emit(L.img, na * per, dst + (size_t)a0 * per);
        wave_sync();   // the image is rebuilt for the next group
    }
}
