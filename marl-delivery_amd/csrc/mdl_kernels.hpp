// mdl_kernels.hpp -- host-visible launchers of the gfx950 kernels (mdl_kernels.hip).
#pragma once
#include "mdl_device.hpp"

namespace mdl {

// sets the thread-local message mdl_last_error() returns (mdl_engine.hip)
void set_error(const char* msg);

struct ShapingConsts {
    float c[9];
};

hipError_t launch_seed(const DevParams& p, const uint32_t* seeds, int wpb, size_t lds, hipStream_t s);
hipError_t launch_reset(const DevParams& p, const int* ids, int n, int wpb, size_t lds, hipStream_t s);
hipError_t launch_tracker_clear(const DevParams& p, const int* ids, int n, hipStream_t s);
// One step per launch.  envs_per_wave is the layout: 1 (k_step: any shape, an id list or the full
// batch), 4 (k_step_rows, mdl_step_rows.hpp: one env per 16-lane row; A <= 8, P <= 64, step_rows_ok)
// or 2 (k_step_halves, mdl_step_halves.hpp: one env per 32-lane half; A == 16, P <= 128,
// step_halves_ok); 4 and 2 step the full batch only (ids == nullptr) and are refused outside their
// shapes.  lds: the layout's per-wave slice (step_lds, step_rows_lds, step_halves_lds).
hipError_t launch_step(const DevParams& p, const uint8_t* actions, int fmt, const int* ids, int n, int auto_reset,
                       double* r, float* sh, uint8_t* done, int wpb, size_t lds, hipStream_t s,
                       int envs_per_wave = 1);
bool step_rows_ok(int A, int P);
size_t step_rows_lds(int P);
bool step_halves_ok(int A, int P);
size_t step_halves_lds(int P);
// The symbol (as rocprof names it) of the step kernel a launch takes: launch_step of that layout, or
// launch_step_obs (obs: the fused step + observation kernel).  It comes from the selection the
// launchers run (select_step, mdl_kernels.hip); bench.py labels its roofline record with it.
// Returns snprintf's count.
int step_kernel_name(const DevParams& p, int envs_per_wave, bool obs, char* out, int cap);
// the step's launch shape (grid, workgroup, LDS, kernel arguments) with an empty kernel
hipError_t launch_step_floor(const DevParams& p, int n, int wpb, size_t lds, hipStream_t s, int envs_per_wave = 1);
hipError_t launch_step_fused(const DevParams& p, const uint8_t* actions, int fmt, const int* ids, int n, int K,
                             int auto_reset, double* r, float* sh, uint8_t* done, int wpb, size_t lds,
                             hipStream_t s);
hipError_t launch_step_obs(const DevParams& p, const uint8_t* actions, int fmt, int n, int auto_reset, double* r,
                           float* sh, uint8_t* done, float* amap, float* avec, float* cmap, float* cvec, int wpb,
                           size_t lds, hipStream_t s);
// mdl_step_episode's one launch (launch_step_obs's shapes): one transition of the envs whose
// `active` byte is set and their observation rows, no reset; a done env's byte is cleared, the
// other envs get zero outputs, filled = 0 and unwritten observation rows.
hipError_t launch_step_episode(const DevParams& p, const uint8_t* actions, int fmt, int n, uint8_t* active, double* r,
                               float* sh, uint8_t* done, uint8_t* filled, float* amap, float* avec, float* cmap,
                               float* cvec, int wpb, size_t lds, hipStream_t s);
// mdl_step_episode in the other shapes, around launch_step(ids) and launch_obs(mask = filled):
// begin: ids[e] = e or -1 (skipped), filled[e] = active[e] != 0, zero r / sh / done rows of the
// envs left out (r, sh may be null); end: active[e] = 0 where filled[e] and done[e].
hipError_t launch_episode_begin(const uint8_t* active, int n, int* ids, uint8_t* filled, double* r, float* sh,
                                uint8_t* done, hipStream_t s);
hipError_t launch_episode_end(uint8_t* active, const uint8_t* filled, const uint8_t* done, int n, hipStream_t s);
// rank_lds > 0 (small builder): bytes of LDS in front of the per-wave slices holding the launch's
// distance-rank table (mdl_obs_small.hpp k_obs_small).  PRECONDITION: envs [env_begin, env_begin+n)
// share one map shape -- the table copied is env_begin's map's.  The engine checks it
// (MdlEngine::launch_obs, mdl_engine.hip) before every call.  mask (device, [n], may be null):
// row w is built only where mask[w] != 0, the other rows stay unwritten.  dtype (OBS_F32 / F16 /
// BF16): the four outputs' element type; the half types run k_obs_small_h / k_obs_h in the same
// launch shape (anything else: hipErrorInvalidValue).
enum : int { OBS_F32 = 0, OBS_F16 = 1, OBS_BF16 = 2 };   // = MDL_OBS_* (mdl_engine.h; checked in mdl_engine.hip)
hipError_t launch_obs(const DevParams& p, int env_begin, int n, void* amap, void* avec, void* cmap, void* cvec,
                      int wpb, size_t lds, hipStream_t s, int rank_lds = 0, const uint8_t* mask = nullptr,
                      int dtype = 0);
// The symbol (as rocprof names it) of the builder launch_obs runs for these arguments, from the
// selection launch_obs launches through (select_obs, mdl_kernels.hip).  Returns snprintf's count,
// -1 for an unknown dtype.
int obs_kernel_name(const DevParams& p, int rank_lds, int dtype, char* out, int cap);
// The window builder (k_ego_maps, mdl_ego.hpp): out [n][A][6][K][K] of `dtype`, K = 2R + 1, for envs
// [env_begin, env_begin + n) of any map shapes.  ego_group: the robots whose windows share one LDS
// image for radius R (0: the slice does not fit `budget`); ego_lds: the per-wave slice for that group.
int ego_group(int A, int P, int maxHW, int R, size_t budget);
size_t ego_lds(int P, int maxHW, int G, int R);
// rows (device uint8 [E], indexed by env id; may be null): env e is built only where rows[e] != 0, the
// rows of the other envs stay unwritten (k_masked_ego_maps); null: every env of the range (k_ego_maps).
hipError_t launch_ego(const DevParams& p, int env_begin, int n, const uint8_t* rows, int R, int dtype, void* out,
                      int wpb, size_t lds, int G, hipStream_t s);
// The same windows of k_alt_obs's idq_obs (k_alt_ego, mdl_alt_ego.hpp): float32 out [n][A][6][K][K];
// rows as launch_ego's (null: every env of the range).  alt_ego_group / alt_ego_lds as ego_group / ego_lds.
int alt_ego_group(int A, int P, int maxHW, int R, size_t budget);
size_t alt_ego_lds(int A, int P, int maxHW, int G, int R);
hipError_t launch_alt_ego(const DevParams& p, int env_begin, int n, const uint8_t* rows, int R, float* out, int wpb,
                          size_t lds, int G, hipStream_t s);
// The critic map on a fixed canvas (k_canvas_maps, mdl_canvas.hpp): out [n][4][Hc][Wc] of `dtype` for envs
// [env_begin, env_begin + n) of any map shapes, each no larger than the canvas (the caller checks it; a
// larger map is cropped, not overrun).  canvas_lds: the per-wave slice for maps of up to maxHW cells.
// rows as launch_ego's (null: every env of the range, k_canvas_maps; else k_masked_canvas_maps).
size_t canvas_lds(int P, int maxHW, int Hc, int Wc);
hipError_t launch_canvas(const DevParams& p, int env_begin, int n, const uint8_t* rows, int Hc, int Wc, int dtype,
                         void* out, int wpb, size_t lds, hipStream_t s);
// A launch's own completion word (host-mapped): every wave of its grid counts itself in the
// running device counter `ctr` (never reset: `base` is its value before the launch) after a
// system-scope release of its stores; the last one writes `value` to `seq`.  seq == nullptr: none;
// ctr == nullptr: a one-wave launch, which writes `value` straight after its release.
struct Publish {
    int32_t* seq = nullptr;
    unsigned* ctr = nullptr;
    unsigned base = 0;
    int32_t value = 0;
    unsigned expect = 0;   // > 0: the number of waves that count themselves (not the whole grid)
};
// A view record carried in the kernel arguments (mdl_host_view_*): two capacity classes, the larger
// sized so the kernel's whole argument block stays well inside the 4 KiB kernarg limit.
constexpr int VIEW_INLINE_SMALL = 256, VIEW_INLINE_WORDS = 768;
template <int CAP>
struct ViewInline {
    int32_t w[CAP];
};
hipError_t launch_view_features_inline(const DevParams& p, const int32_t* rec, int words, int a, int T, int MO,
                                      int MP, int MR, int MPs, int MPc, int MPsc, int NSmax, int HW, float* obs,
                                      float* vec, float* gmap, float* gvec, size_t lds, hipStream_t s,
                                      const Publish& pb);
// the result comes back in the completion word's second half (pb.seq 8-byte aligned)
hipError_t launch_view_shaped_inline(const int32_t* rec, int words, int co, int ao, double g, const ShapingConsts& C,
                                     int NSmax, size_t lds, hipStream_t s, const Publish& pb);
unsigned grid_waves(int n, int wpb);   // waves of a 256-thread-block launch of wpb views per block
hipError_t launch_views_features(const DevParams& p, const int32_t* views, const int64_t* offs, int n,
                                 const int32_t* agent_idx, int T, int MO, int MP, int MR, int MPs, int MPc, int MPsc,
                                 int NSmax, int HW, float* obs, float* vec, float* gmap, float* gvec, int wpb,
                                 size_t lds, hipStream_t s, const Publish& pb = Publish{});
hipError_t launch_views_shaped(const DevParams& p, const int32_t* prev, const int64_t* prev_offs, const int32_t* cur,
                               const int64_t* cur_offs, const uint8_t* acts, const int64_t* act_offs, const double* g,
                               int n, const ShapingConsts& C, float* out, int wpb, size_t lds, int NSmax,
                               hipStream_t s, const Publish& pb = Publish{});
// the dict-API mailbox's output rows (host-mapped memory; row w = the w-th env of a call)
struct MailRows {
    int32_t* seq;      // completion word, written last
    int32_t* robots;   // [E][A][3]
    int32_t* pkgs;     // [E][P][8]
    int32_t* t;        // [E]
    double* total;     // [E]
    int32_t* rterms;   // [E] RT_* bits
};
hipError_t launch_publish(int32_t* seq, int32_t value, hipStream_t s);
// mdl_mail_step in one launch: the step (action codes, rows [0, n) = envs ids[w] or w), its rows
// into the mailbox, the completion word `seq` once all n waves have counted themselves in `ctr`
hipError_t launch_step_mail(const DevParams& p, const uint8_t* codes, const int* ids, int n, int auto_reset, double* r,
                            float* sh, uint8_t* done, int wpb, size_t lds, const MailRows& m, unsigned* ctr,
                            unsigned base, int32_t seq, hipStream_t s);
unsigned mail_export_waves(int n);   // waves of one k_mail_export launch over n envs
hipError_t launch_mail_export(const DevParams& p, const int32_t* ids, int n, const MailRows& m, unsigned* ctr,
                              unsigned base, int32_t seq, hipStream_t s);
hipError_t launch_export(const DevParams& p, int32_t* robots, int32_t* pkgs, int32_t* t, double* total,
                         int32_t* tracker, int32_t* tracker_data, hipStream_t s);
// k_episode_results over all p.E envs: total_reward, delivered package slots, t (each may be null)
hipError_t launch_episode_results(const DevParams& p, double* total, int32_t* delivered, int32_t* steps,
                                  hipStream_t s);
// k_avail_actions over all p.E envs: uint8 [E][A][15]; active (device uint8 [E]) may be null
hipError_t launch_avail_actions(const DevParams& p, const uint8_t* active, uint8_t* avail, hipStream_t s);

// Greedy agent record layout (mdl_greedy.hip): per env `stride` bytes.
struct GreedyLayout {
    int A, cap, stride, list_off, free_off, lds_stride;
    int64_t tab_off[MAX_MAPS];  // BFS table of map m: tables + tab_off[m], [HW goal][HW cell] u16
};
hipError_t launch_bfs_table(const uint8_t* grid, int H, int W, uint16_t* table, hipStream_t s);
hipError_t launch_greedy_init(const DevParams& p, const GreedyLayout& g, unsigned char* gs, const int* ids, int n,
                              hipStream_t s);
// mask (device uint8 [E], may be null; then ids must be null and n == p.E): an env whose byte is 0
// gets the all-zero action row and nothing else of it is read or written
hipError_t launch_greedy_act(const DevParams& p, const GreedyLayout& g, unsigned char* gs, const uint16_t* tables,
                             const int* ids, int n, uint8_t* actions, hipStream_t s, const uint8_t* mask = nullptr);

hipError_t launch_alt_obs(const DevParams& p, int env_begin, int n, float* idq, float* qst, int oh, int ow, int wpb,
                          size_t lds, hipStream_t s);
hipError_t launch_views_alt(const DevParams& p, const int32_t* views, const int64_t* offs, int n,
                            const int32_t* agent_idx, float* idq, float* qst, int oh, int ow, int wpb, size_t lds,
                            int NSmax, hipStream_t s);
hipError_t launch_views_idq_reward(const int32_t* prev, const int64_t* prev_offs, const int32_t* cur,
                                   const int64_t* cur_offs, const uint8_t* ops, const int64_t* op_offs,
                                   int ops_are_ints, int n, double* out, int wpb, size_t lds, int NSmax,
                                   hipStream_t s);
// k_alt_transition over all p.E envs; pre: the caller's record of alt_pre_size(E, A) bytes
hipError_t launch_alt_transition(const DevParams& p, const uint8_t* acts, int fmt, int ops_are_ints,
                                 const uint8_t* mask, void* pre, double* r_idq, float* idq, float* qst, int oh, int ow,
                                 int wpb, size_t lds, hipStream_t s);
size_t alt_pre_size(int E, int A);
// k_cycle_begin over all p.E envs: the masked reset and the observations of the reset rows
hipError_t launch_cycle_begin(const DevParams& p, uint8_t* done, uint8_t* completed, double* c_return,
                              int32_t* c_steps, float* idq, float* qst, int oh, int ow, int wpb, size_t lds,
                              hipStream_t s);
size_t cycle_begin_lds(int P, int HW);
size_t alt_obs_lds(int P, int HW);
size_t views_alt_lds(int NSmax, int HW);

size_t step_lds(int P);
size_t obs_lds(int A, int P, int HW, int MO, int MP, int MR, int MPs);
int obs_plane_words(int A, int HW);
size_t obs_lds_small(int A, int HW, int P, int MO, int MP);
bool obs_use_small(int A, int P, int key7_dsh, int maxHW, int MO, int MP);
size_t views_lds(int NSmax, int HW, int MO, int MPc, int MR, int MPsc);
size_t views_shaped_lds(int NSmax);

}  // namespace mdl
