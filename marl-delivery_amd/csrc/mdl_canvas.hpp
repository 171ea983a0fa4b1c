// mdl_canvas.hpp -- the critic map on a fixed canvas (mdl_build_obs_canvas, k_canvas_maps).
//
// For a canvas (Hc, Wc) with Hc >= H and Wc >= W, anchored at the map's top-left cell:
//   canvas[ch][i][j] = convert_global_state(...)[0][ch][i][j]   for i < H and j < W   (MAPPO/helper.py:167-197)
//                    = 1.0 in channel 0, 0.0 in channels 1-3    elsewhere
// An off-map cell reads as an obstacle: the windows' rule (mdl_ego.hpp).  The output shape [4][Hc][Wc]
// does not depend on the map, so one launch may cross map shapes: every wave reads its own env's MapDesc.
// With (Hc, Wc) == (H, W) the canvas is the builders' critic_map.
//
// One wave per env.  LDS per wave (canvas_lds_bytes):
//   tracker slots   obs_pre_bytes(P)            (stage_tracker, as the other builders)
//   bits            uint32[4][NW]               the critic map's cell bitsets: BS_GRID, BS_ROBOT, BS_WSTART,
//                                               BS_ATARGET -- channel ch is set ch
//   image           uint32[canvas_image_words]  flat bit image of the env's 4 * Hc * Wc output elements
// The prepare is the windows' ego_prepare less what the critic map does not use: no BS_MULTI set (and no
// atomic's return value to wait for), no rcell / rtgt (512 B of the slice) and no carrier lookup -- channel 3
// takes a carried package's target from the tracker's in-transit entry, not from the robot.
// A canvas row is a Wc-bit field of the image (bit ((ch * Hc + i) * Wc + j: element order of the output):
// the map row's W bits, funnel-shifted out of the bitset 32 at a time (ego_bits32), then the pad bits.
// No canvas coordinate indexes LDS unclamped: a row i >= H and a column c0 >= W are constants that read
// nothing; for i < H and c0 < W the bit index i * W + c0 is below H * W, and ego_bits32 clamps both word
// indices to [0, NW) whatever it is given; the bits past the row's last column are masked.  The image is
// written at word k <= (4 * Hc * Wc + 31) / 32, which the host sizes the slice for (canvas_image_words).
// The kernels have no workgroup barrier.
//
// Included by mdl_kernels.hip, inside namespace mdl, after mdl_ego.hpp (ego_bits32, ego_emit).
#pragma once

static_assert(BS_GRID == 0 && BS_ROBOT == 1 && BS_WSTART == 2 && BS_ATARGET == 3,
              "critic-map channel ch is bitset ch (convert_global_state's order)");

// words of the image: the bits, and one word more (the emitters' funnel shifts read the word after the last)
__host__ __device__ inline int canvas_image_words(int Hc, int Wc) { return (4 * Hc * Wc + 31) / 32 + 1; }

__host__ __device__ inline size_t canvas_lds_bytes(int P, int HW, int Hc, int Wc) {
    return obs_pre_bytes(P) + align16(sizeof(uint32_t) * 4 * (size_t)((HW + 31) / 32)) +
           align16(sizeof(uint32_t) * (size_t)canvas_image_words(Hc, Wc));
}

// The four cell bitsets of the critic map (feat_prepare's, as ego_prepare builds them).  Robots come in on
// lanes (lane a < A): cell packed r | c << 8.
template <class Trk>
__device__ __forceinline__ void canvas_prepare(const Trk& trk, uint32_t* bits, const uint32_t* gridbits, int NW, int W,
                                               int A, int NS, int t, int cell) {
    const int lane = lane_id();
    const unsigned nbits = (unsigned)NW << 5;
    for (int w = lane; w < NW; w += WAVE) {
        bits[BS_GRID * NW + w] = gridbits[w];
        bits[BS_ROBOT * NW + w] = 0;
        bits[BS_WSTART * NW + w] = 0;
        bits[BS_ATARGET * NW + w] = 0;
    }
    wave_sync();
    if (lane < A) {
        const unsigned rc = (unsigned)(cell_r(cell) * W + cell_c(cell));
        if (rc < nbits) atomicOr(&bits[BS_ROBOT * NW + (rc >> 5)], 1u << (rc & 31));
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
                if (ci < nbits) atomicOr(&bits[BS_WSTART * NW + (ci >> 5)], 1u << (ci & 31));
            }
            if (wt || it) {
                const unsigned ci = (unsigned)(cell_r(tg) * W + cell_c(tg));
                if (ci < nbits) atomicOr(&bits[BS_ATARGET * NW + (ci >> 5)], 1u << (ci & 31));
            }
        }
    }
    wave_sync();
}

// The 32 bits of canvas row i of channel ch from column c0 on (bits past the canvas row's end are
// don't-care): map columns c0 .. W - 1 from the bitset, the pad after them.
__device__ __forceinline__ uint32_t canvas_bits32(const uint32_t* bits, int NW, int H, int W, int ch, int i, int c0) {
    const uint32_t pad = ch == 0 ? ~0u : 0u;
    if ((unsigned)i >= (unsigned)H || c0 >= W) return pad;   // a row below the map, columns right of it
    const int nv = W - c0;   // >= 1 map columns from c0 on
    const uint32_t cm = nv >= 32 ? ~0u : (1u << nv) - 1u;
    return (ego_bits32(bits + ch * NW, NW, i * W + c0) & cm) | (pad & ~cm);
}

// The env's canvas as a flat bit image (build_flat's packing with Wc-bit rows): lane k builds word k from
// the rows that overlap it, walking (channel, row) in step.  Every pass takes the rest of a row or fills
// the word, so the walk ends.
__device__ __forceinline__ void canvas_build_image(const uint32_t* bits, uint32_t* img, int NW, int H, int W, int Hc,
                                                   int Wc) {
    const int lane = lane_id();
    const int nrow = 4 * Hc, nfw = (nrow * Wc + 31) >> 5;
    const float inv_w = 1.0f / (float)Wc, inv_h = 1.0f / (float)Hc;
    for (int k = lane; k < nfw; k += WAVE) {
        const int g0 = k << 5;   // < 2^23: fdivi is exact
        int p = fdivi(g0, Wc, inv_w);
        int c0 = g0 - p * Wc;
        int ch = fdivi(p, Hc, inv_h);
        int i = p - ch * Hc;
        uint32_t out = 0;
        int pos = 0;
        while (pos < 32 && p < nrow) {
            const int nb = min(32 - pos, Wc - c0);   // >= 1
            const uint32_t m = nb >= 32 ? ~0u : (1u << nb) - 1u;
            out |= (canvas_bits32(bits, NW, H, W, ch, i, c0) & m) << pos;
            pos += nb;
            c0 += nb;
            if (c0 == Wc) {
                c0 = 0;
                p++;
                if (++i == Hc) {
                    i = 0;
                    ch++;
                }
            }
        }
        img[k] = out;
    }
    if (lane == 0) img[nfw] = 0u;   // the word the emitters read after the last
    wave_sync();
}

// Env e's canvas at out + w * 4 * Hc * Wc, in the wave's LDS slice at base.
template <bool STALE, class OT>
__device__ __forceinline__ void canvas_env(const DevParams& p, int e, int w, int Hc, int Wc, OT* __restrict__ out,
                                           unsigned char* base) {
    const int lane = lane_id();
    const int A = p.A, P = p.P;
    ObsLdsPre S = obs_pre_carve(base, P);
    const MapDesc md = p.maps[p.env_map ? p.env_map[e] : 0];
    const int H = md.H, W = md.W, NW = (H * W + 31) >> 5;
    uint32_t* bits = (uint32_t*)(base + obs_pre_bytes(P));
    uint32_t* img = (uint32_t*)(base + obs_pre_bytes(P) + align16(sizeof(uint32_t) * 4 * (size_t)NW));
    const int t = p.es[e].t;
    const uint32_t rv = lane < A ? p.rob[(size_t)e * A + lane] : 0u;
    stage_tracker<STALE>(p, e, P, lane, S);
    canvas_prepare(staged_tracker<STALE>(S, P), bits, p.gridbits + md.bits_off, NW, W, A, P, t, rob_cell(rv));
    canvas_build_image(bits, img, NW, H, W, Hc, Wc);
    const int per = 4 * Hc * Wc;   // elements per env
    [[clang::always_inline]] ego_emit(img, per, out + (size_t)w * per);
}

// out [n][4][Hc][Wc] of envs [env_begin, env_begin + n).
template <bool STALE, class OT>
__global__ __launch_bounds__(256) void k_canvas_maps(DevParams p, int env_begin, int n, int Hc, int Wc,
                                                     OT* __restrict__ out, int wpb, int lds_stride) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int wave = wave_id();
    const int w = xcd_block() * wpb + wave;
    if (wave >= wpb || w >= n) return;
    canvas_env<STALE, OT>(p, env_begin + w, w, Hc, Wc, out, smem + (size_t)wave * lds_stride);
}

// k_canvas_maps under a row mask: rows (uint8 [E], indexed by env id, non-zero = build) marks the envs to
// build.  The wave of an unmarked env leaves after one byte load, before it touches LDS, and writes
// nothing.  A sibling on the same device function, as k_masked_ego_maps is k_ego_maps's: the unmasked
// kernel carries no mask argument or test.
template <bool STALE, class OT>
__global__ __launch_bounds__(256) void k_masked_canvas_maps(DevParams p, int env_begin, int n, int Hc, int Wc,
                                                            OT* __restrict__ out, int wpb, int lds_stride,
                                                            const uint8_t* __restrict__ rows) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int wave = wave_id();
    const int w = xcd_block() * wpb + wave;
    if (wave >= wpb || w >= n) return;
    const int e = env_begin + w;
    if (__builtin_amdgcn_readfirstlane((int)rows[e]) == 0) return;   // wave-uniform: one byte, before any LDS use
    canvas_env<STALE, OT>(p, e, w, Hc, Wc, out, smem + (size_t)wave * lds_stride);
}
