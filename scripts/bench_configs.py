"""Secondary measurements for BASELINE.json configs 3-5 (single GPU slices).

  --config 1   map1, A=5, ONE env driven through the dict API by a random agent (plumbing)
  --config 3   map1, A=5, E=16384: step + full observation build every step
               (actor 6ch map + vector 52 (MO=4, MP=5), critic 4ch map + vector 1301)
  --config 3b  as 3 with the 1007-dim actor vector (MO=MP=100)
  --config 4   map1..map5 mixed, A=5, E=65536/8 per GPU (one GPU's shard), step only
  --config 5   synthetic 64x64, A=16, P=100, E=131072/8 per GPU, step; full observations per
               chunk of 4096 envs (MDL_OBS_CHUNK)
  --config rollout / rollout_graph   MAPPO rollout on the device
  --obs-dtype       float16 / bfloat16 observations: configs 3 / 3b time step_obs and build_obs for float32
                    and the half types in one process; rollout / rollout_graph collect in that type
  --ego-radius      R (or several): configs 3 / 5 time build_obs_ego (float32 and bfloat16, all envs in one
                    call) beside the full actor maps' build_obs in one process
  --ego-active      FRACTION (or several), with --ego-radius: also time build_obs_ego_masked under a fixed
                    mask with that share of the envs set (1 = all set: the mask's own cost)
  --ego-collect     E, with --ego-radius and --config 5: one QmixCollector(ego_radius=R).collect(graph=True)
                    of E envs on config 5's shape with a linear agent, instead of the builder's times
  --alt-ego-radius  R (or several), with --config 5: build_obs_alt_ego (all envs, and masks of 1/2 and 1/8 of them)
                    beside build_obs_ego in float32 and the full idq_obs build, in one process
  --config alt      IDQ/qmix featurizers (§8(f)2)
  --config greedy   batched greedy baseline (§8(f)3)
  --canvas          HC WC: configs 3 / 5 time build_obs_canvas of the critic map (the map's own shape and HC x WC,
                    float32 and bfloat16, all envs in one call) beside build_obs's critic_map; config 4 times a
                    graphed mixed-map MappoRollout(ego_radius=5, canvas=) beside the single-shape ego rollout
  --qmix            QMIX episode collection: the masked step against the full step, and one collector
                    step against the host-driven subset loop
  --idq             IDQ transition collection: alt_transition against build_obs_alt, and one collector
                    step against the host-driven loop it replaces
  --qmix-cycle      map-QMIX cycle collection: cycle_begin against reset + build_obs_alt, the joint
                    replay append, and one collector step against the host-driven loop
  --eval            device-resident evaluation: the greedy agent's mask, episode_results against the
                    read_state export, and one greedy evaluation against the host-driven loop
  --avail           the valid-action mask: avail_actions per call (null, all-ones and all-zero masks)
                    beside episode_results and the all-zero greedy_actions_masked, and one QMIX collect
                    with the mask on and off; --avail-collect off: the collect alone, without
                    the option (it runs on a build that predates it)

Prints one JSON line per config with per-kernel HIP-event times and the
algorithmic-bytes roofline of SURVEY.md §8(d).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "marl-delivery_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM = 8000.0


def timed(fn, n):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for k in range(n):
        fn(k)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1e3  # us per call


def graph_timed(fn, G, reps):
    """us per step of G captured calls fn(0..G-1) replayed `reps` times (after one untimed
    replay): the kernels without the host launch path."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        fn(0)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            for k in range(G):
                fn(k)
    torch.cuda.synchronize()
    g.replay()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / (G * reps) * 1e3


def run(cfg, steps, warmup):
    import marl_gpu
    from marl_gpu.maps import grid_array, load_map, map_path
    dev = torch.device("cuda", 0)
    if cfg in ("3", "3b"):
        E, A, P, T = 16384, 5, 50, 500
        mo, mp = (4, 5) if cfg == "3" else (100, 100)
        env = marl_gpu.BatchedEnv(grid_array(load_map(map_path("map1.txt"))), E, A, P, T, seed=42, tracker="mappo",
                                  max_other_robots=mo, max_packages_obs=mp)
        groups = [(0, E)]
    elif cfg == "4":
        E, A, P, T = 65536 // 8, 5, 50, 500
        maps = [grid_array(load_map(map_path(f"map{i}.txt"))) for i in range(1, 6)]
        sizes = [E // 5 + (1 if i < E % 5 else 0) for i in range(5)]
        env_map = np.concatenate([np.full(s, i) for i, s in enumerate(sizes)])
        env = marl_gpu.BatchedEnv(maps, E, A, P, T, seed=42, env_map=env_map, tracker="mappo", max_packages_obs=5)
        starts = np.cumsum([0] + sizes)
        groups = [(int(starts[i]), int(sizes[i])) for i in range(5)]
    else:
        E, A, P, T = 131072 // 8, 16, 100, 500
        env = marl_gpu.BatchedEnv(grid_array(load_map(map_path("synthetic64.txt"))), E, A, P, T, seed=7,
                                  tracker="mappo", max_other_robots=15, max_packages_obs=20, max_robots_state=16,
                                  max_packages_state=100)
        groups = [(0, E)]
    env.reset()
    gen = torch.Generator(device=dev).manual_seed(0)
    G = 50
    acts = torch.randint(0, 15, (G, E, A), generator=gen, device=dev, dtype=torch.int32).to(torch.uint8)
    out = {}
    bufs = None
    if cfg in ("3", "3b"):
        bufs = env.obs_buffers()
    for k in range(warmup):
        env.step(acts[k % G])
    step_eager_us = timed(lambda k: env.step(acts[k % G]), steps)
    r = torch.zeros(E, dtype=torch.float64, device=dev)
    sh = torch.zeros(E, dtype=torch.float32, device=dev)
    dn = torch.zeros(E, dtype=torch.uint8, device=dev)
    step_us = graph_timed(lambda k: env.step(acts[k % G], out=(r, sh, dn)), G, max(1, steps // G))
    out["step_us"] = step_us          # hipGraph-replayed steps (the kernel path)
    out["step_eager_us"] = step_eager_us
    out["agent_steps_per_s_step_only"] = E * A / (step_us * 1e-6)
    step_bytes = (9 * A + 10 * P + 41) * E
    out["step_roofline"] = {"achieved_GBs": step_bytes / (step_us * 1e-6) / 1e9, "frac": step_bytes / (step_us * 1e-6) / 1e9 / HBM}
    if bufs is not None:
        for k in range(3):
            env.build_obs(out=bufs)
        obs_us = timed(lambda k: env.build_obs(out=bufs), max(20, steps // 5))
        H = W = 10
        obs_bytes = E * 4 * (A * 6 * H * W + A * env.actor_vec_dim + 4 * H * W + env.critic_vec_dim)
        out["obs_us"] = obs_us
        out["obs_write_bytes"] = obs_bytes
        out["obs_roofline"] = {"achieved_GBs": obs_bytes / (obs_us * 1e-6) / 1e9,
                               "frac": obs_bytes / (obs_us * 1e-6) / 1e9 / HBM}
        both = timed(lambda k: (env.step(acts[k % G]), env.build_obs(out=bufs)), max(20, steps // 5))
        out["step_plus_obs_eager_us"] = both
        # hipGraph-replayed: step + build_obs as two launches, and mdl_step_obs (one launch)
        both_g = graph_timed(lambda k: (env.step(acts[k % G], out=(r, sh, dn)), env.build_obs(out=bufs)), 10,
                             max(1, steps // 50))
        try:
            fused_g = graph_timed(lambda k: env.step_obs(acts[k % G], out=(r, sh, dn), obs_out=bufs), 10,
                                  max(1, steps // 50))
        except AttributeError:   # an older profiling build without mdl_step_obs (same-box A/B)
            fused_g = float("nan")
        out["step_plus_obs_us"] = both_g
        out["step_obs_fused_us"] = fused_g
        out["agent_steps_per_s_with_obs"] = E * A / (fused_g * 1e-6)
        out["step_obs_roofline"] = {"achieved_GBs": (obs_bytes + step_bytes) / (fused_g * 1e-6) / 1e9,
                                    "frac": (obs_bytes + step_bytes) / (fused_g * 1e-6) / 1e9 / HBM}
    if cfg == "5":
        # the full observations (actor 6 x 64 x 64 maps for 16 agents, vectors
        # MO = 15 / MP = 20, critic map + MR = 16 / MPs = 100 vector) are 1.65 MB per env-step, so they
        # are built and reported per chunk of envs (general k_obs builder: A > 8, P > 64)
        H = W = 64
        chunk = int(os.environ.get("MDL_OBS_CHUNK", "4096"))
        cb = env.obs_buffers(chunk, H, W)
        per_env = 4 * (A * 6 * H * W + A * env.actor_vec_dim + 4 * H * W + env.critic_vec_dim)
        for k in range(2):
            env.build_obs(0, chunk, out=cb)
        nchunks = E // chunk
        reps = 2
        chunk_us = timed(lambda k: env.build_obs((k % nchunks) * chunk, chunk, out=cb), nchunks * reps)
        out["obs_chunk_envs"] = chunk
        out["obs_chunk_us"] = chunk_us
        out["obs_bytes_per_env_step"] = per_env
        out["obs_chunk_roofline"] = {"achieved_GBs": per_env * chunk / (chunk_us * 1e-6) / 1e9,
                                     "frac": per_env * chunk / (chunk_us * 1e-6) / 1e9 / HBM}
        out["obs_all_envs_us"] = chunk_us * nchunks
        out["agent_steps_per_s_step_plus_obs"] = E * A / ((step_us + chunk_us * nchunks) * 1e-6)
        del cb
    out.update(config=cfg, envs=E, agents=A, packages=P, T=T, groups=groups)
    print(json.dumps(out), flush=True)
    env.close()


OBS_DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


def run_obs_dtype(cfg, steps, warmup, names, rounds=3):
    """Config 3 / 3b with half-precision observations ("Half-precision observations"):
    in one process, on one engine, ``step_obs`` and ``build_obs`` alone for float32 and for each
    half type of ``names`` -- the config 3 leg's warm-up and its hipGraph-replayed timed region (10
    captured calls), each graph captured once and the types replayed in turn, ``rounds`` times.
    float32 ``step_obs`` is the fused kernel; a half ``step_obs`` is the step launch + the builder's."""
    import marl_gpu
    from marl_gpu.maps import grid_array, load_map, map_path
    dev = torch.device("cuda", 0)
    E, A, P, T = 16384, 5, 50, 500
    mo, mp = (4, 5) if cfg == "3" else (100, 100)
    env = marl_gpu.BatchedEnv(grid_array(load_map(map_path("map1.txt"))), E, A, P, T, seed=42, tracker="mappo",
                              max_other_robots=mo, max_packages_obs=mp)
    env.reset()
    gen = torch.Generator(device=dev).manual_seed(0)
    G, C = 50, 10
    acts = torch.randint(0, 15, (G, E, A), generator=gen, device=dev, dtype=torch.int32).to(torch.uint8)
    for k in range(warmup):
        env.step(acts[k % G])
    r = torch.zeros(E, dtype=torch.float64, device=dev)
    sh = torch.zeros(E, dtype=torch.float32, device=dev)
    dn = torch.zeros(E, dtype=torch.uint8, device=dev)
    names = ["float32"] + [n for n in names if n != "float32"]
    elems = E * (A * 6 * 100 + A * env.actor_vec_dim + 4 * 100 + env.critic_vec_dim)
    graphs = {}
    for n in names:
        dt = OBS_DTYPES[n]
        bufs = env.obs_buffers(dtype=dt)

        def steps_(bufs=bufs, dt=dt):
            for k in range(C):
                env.step_obs(acts[k % G], out=(r, sh, dn), obs_out=bufs, obs_dtype=dt)

        def builds_(bufs=bufs, dt=dt):
            for k in range(C):
                env.build_obs(out=bufs, dtype=dt)

        graphs[n] = (_graph_of(steps_), _graph_of(builds_), bufs)
    reps = max(1, steps // 50)
    res = {n: {"step_obs_us": [], "build_obs_us": []} for n in names}
    for _ in range(rounds):
        for n in names:
            res[n]["step_obs_us"].append(_replay_us(graphs[n][0], reps, C))
            res[n]["build_obs_us"].append(_replay_us(graphs[n][1], reps, C))
    for n in names:
        b = elems * (4 if n == "float32" else 2)
        best = min(res[n]["build_obs_us"])
        res[n].update(obs_write_bytes=b, step_obs_launches=1 if n == "float32" else 2,
                      build_obs_roofline_frac=b / (best * 1e-6) / 1e9 / HBM)
    print(json.dumps({"config": cfg + ":obs_dtype", "envs": E, "agents": A, "packages": P, "rounds": rounds,
                      "replays": reps, "calls_per_graph": C, "dtypes": res}), flush=True)
    env.close()


def ego_mask(E, frac):
    """A fixed mask with the share `frac` of E envs set, spread evenly: env e is set where floor((e + 1) * frac)
    passes floor(e * frac) (1/2: every second env, 1/8: every eighth)."""
    e = np.arange(E, dtype=np.int64)
    return (np.floor((e + 1) * frac + 1e-9) > np.floor(e * frac + 1e-9)).astype(np.uint8)


def run_ego(cfg, radii, steps, warmup, rounds=3, active=()):
    """Robot-centred actor-map windows ("Egocentric actor windows"), config 3 or 5: in one
    process, on one engine, ``build_obs_ego`` over all of the rank's envs in one call, float32 and
    bfloat16 at each radius, beside the existing full-map ``build_obs(which=("actor_map",))`` (float32;
    config 5: per chunk of 4,096 envs, as its usual leg builds them).  Every figure is a hipGraph of 10
    captured calls, each graph captured once and replayed in turn, ``rounds`` times.  ``active``: shares of
    the envs; for each, ``build_obs_ego_masked`` under ``ego_mask`` is timed the same way."""
    import marl_gpu
    from marl_gpu.maps import grid_array, load_map, map_path
    dev = torch.device("cuda", 0)
    if cfg == "3":
        E, A, P, T, H = 16384, 5, 50, 500, 10
        env = marl_gpu.BatchedEnv(grid_array(load_map(map_path("map1.txt"))), E, A, P, T, seed=42, tracker="mappo",
                                  max_other_robots=4, max_packages_obs=5)
        chunk = E
    elif cfg == "5":
        E, A, P, T, H = 131072 // 8, 16, 100, 500, 64
        env = marl_gpu.BatchedEnv(grid_array(load_map(map_path("synthetic64.txt"))), E, A, P, T, seed=7,
                                  tracker="mappo", max_other_robots=15, max_packages_obs=20, max_robots_state=16,
                                  max_packages_state=100)
        chunk = int(os.environ.get("MDL_OBS_CHUNK", "4096"))
    else:
        raise SystemExit("--ego-radius goes with --config 3 or --config 5")
    env.reset()
    gen = torch.Generator(device=dev).manual_seed(0)
    G, C = 50, 10
    acts = torch.randint(0, 15, (G, E, A), generator=gen, device=dev, dtype=torch.int32).to(torch.uint8)
    for k in range(warmup):
        env.step(acts[k % G])
    nchunks = E // chunk
    full = {"actor_map": torch.empty((chunk, A, 6, H, H), dtype=torch.float32, device=dev)}

    def full_():
        for k in range(C):
            env.build_obs((k % nchunks) * chunk, chunk, out=full, which=("actor_map",))

    graphs = {"full_map_float32": (_graph_of(full_), full, chunk * A * 6 * H * H * 4)}
    for R in radii:
        for n in ("float32", "bfloat16"):
            buf = env.ego_buffers(R, dtype=OBS_DTYPES[n])

            def ego_(buf=buf, R=R, n=n):
                for k in range(C):
                    env.build_obs_ego(R, out=buf, dtype=OBS_DTYPES[n])

            graphs[f"ego_r{R}_{n}"] = (_graph_of(ego_), buf, buf.numel() * buf.element_size())
            for frac in active:
                rows = torch.from_numpy(ego_mask(E, frac)).to(dev)
                nset = int(rows.sum())

                def masked_(buf=buf, R=R, n=n, rows=rows):
                    for k in range(C):
                        env.build_obs_ego_masked(R, rows, out=buf, dtype=OBS_DTYPES[n])

                graphs[f"ego_r{R}_{n}_masked_{frac:g}"] = (_graph_of(masked_), (buf, rows),
                                                           buf.numel() * buf.element_size() // E * nset)
    reps = max(1, steps // 50)
    t = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, (g, _, _) in graphs.items():
            t[k].append(_replay_us(g, reps, C))
    res = {}
    for k, (_, _, b) in graphs.items():
        best = min(t[k])
        res[k] = {"us_per_call": t[k], "envs_per_call": chunk if k.startswith("full") else E, "bytes_written": b,
                  **({"envs_set": int(graphs[k][1][1].sum())} if "_masked_" in k else {}),
                  "achieved_GBs": b / (best * 1e-6) / 1e9, "frac_of_8TBs": b / (best * 1e-6) / 1e9 / HBM}
    res["full_map_float32"]["us_all_envs"] = [x * nchunks for x in t["full_map_float32"]]
    print(json.dumps({"config": cfg + ":ego", "envs": E, "agents": A, "packages": P, "map": [H, H], "radii": list(radii),
                      "rounds": rounds, "replays": reps, "calls_per_graph": C, "builds": res}), flush=True)
    env.close()


def run_alt_ego(radii, steps, warmup, rounds=3, active=(0.5, 0.125)):
    """Robot-centred IDQ / map-QMIX windows ("Egocentric IDQ windows") on config 5's shard shape
    (synthetic 64x64, A = 16, P = 100, 16,384 envs, the IDQ / qmix trainers' fresh tracker): in one process, on
    one engine, at each radius ``build_obs_alt_ego`` over all envs, the same under ``ego_mask`` at the shares
    ``active`` and ``build_obs_ego`` in float32 (the same bytes from the 0/1-only kernel), beside the full
    ``build_obs_alt(which=("idq_obs",))`` per chunk of 4,096 envs, scaled to the shard.  Every figure is a
    hipGraph of 10 captured calls, each graph captured once and replayed in turn, ``rounds`` times."""
    import marl_gpu
    from marl_gpu.maps import grid_array, load_map, map_path
    dev = torch.device("cuda", 0)
    E, A, P, T, H = 131072 // 8, 16, 100, 500, 64
    env = marl_gpu.BatchedEnv(grid_array(load_map(map_path("synthetic64.txt"))), E, A, P, T, seed=7, tracker="fresh",
                              max_other_robots=15, max_packages_obs=20, max_robots_state=16, max_packages_state=100)
    chunk = int(os.environ.get("MDL_OBS_CHUNK", "4096"))
    env.reset()
    gen = torch.Generator(device=dev).manual_seed(0)
    G, C = 50, 10
    acts = torch.randint(0, 15, (G, E, A), generator=gen, device=dev, dtype=torch.int32).to(torch.uint8)
    for k in range(warmup):
        env.step(acts[k % G])
    nchunks = E // chunk
    full = {"idq_obs": torch.empty((chunk, A, 6, H, H), dtype=torch.float32, device=dev)}

    def full_():
        for k in range(C):
            env.build_obs_alt((k % nchunks) * chunk, chunk, out=full, which=("idq_obs",))

    graphs = {"full_idq_obs": (_graph_of(full_), None, chunk * A * 6 * H * H * 4)}
    keep = [full]   # what the graphs write: a replay after its tensor was freed writes through a stale address
    for R in radii:
        K = 2 * R + 1
        buf = torch.empty((E, A, 6, K, K), dtype=torch.float32, device=dev)
        keep.append(buf)
        nbytes = buf.numel() * 4

        def alt_(buf=buf, R=R, rows=None):
            for k in range(C):
                env.build_obs_alt_ego(R, rows=rows, out=buf)

        def ego_(buf=buf, R=R):
            for k in range(C):
                env.build_obs_ego(R, out=buf)

        graphs[f"alt_ego_r{R}"] = (_graph_of(alt_), None, nbytes)
        for frac in active:
            rows = torch.from_numpy(ego_mask(E, frac)).to(dev)
            graphs[f"alt_ego_r{R}_masked_{frac:g}"] = (_graph_of(lambda f=alt_, rows=rows: f(rows=rows)), rows,
                                                       nbytes // E * int(rows.sum()))
        graphs[f"ego_r{R}_float32"] = (_graph_of(ego_), None, nbytes)
    reps = max(1, steps // 50)
    t = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, (g, _, _) in graphs.items():
            t[k].append(_replay_us(g, reps, C))
    res = {}
    for k, (_, rows, b) in graphs.items():
        best = min(t[k])
        res[k] = {"us_per_call": t[k], "envs_per_call": chunk if k.startswith("full") else E, "bytes_written": b,
                  **({"envs_set": int(rows.sum())} if rows is not None else {}),
                  "achieved_GBs": b / (best * 1e-6) / 1e9, "frac_of_8TBs": b / (best * 1e-6) / 1e9 / HBM}
    res["full_idq_obs"]["us_all_envs"] = [x * nchunks for x in t["full_idq_obs"]]
    full_all = min(res["full_idq_obs"]["us_all_envs"])
    for R in radii:
        best = min(t[f"alt_ego_r{R}"])
        res[f"alt_ego_r{R}"]["of_full_idq_obs"] = best / full_all
        res[f"alt_ego_r{R}"]["of_ego_float32"] = best / min(t[f"ego_r{R}_float32"])
    print(json.dumps({"config": "5:alt_ego", "envs": E, "agents": A, "packages": P, "map": [H, H], "radii": list(radii),
                      "rounds": rounds, "replays": reps, "calls_per_graph": C, "builds": res}), flush=True)
    del graphs, keep
    env.close()


def run_ego_collect(E, R, steps):
    """One ``QmixCollector(ego_radius=R).collect(graph=True)`` on config 5's shape (synthetic 64x64, A = 16,
    P = 100, T = 500) at E envs, with a linear agent on the actor vector: us per env-step of whole collects
    (every env counted for all L steps, as the loop runs them)."""
    import marl_gpu
    from marl_gpu.maps import grid_array, load_map, map_path
    from marl_gpu.qmix_rollout import QmixCollector
    dev = torch.device("cuda", 0)
    A, P, T = 16, 100, 500
    env = marl_gpu.BatchedEnv(grid_array(load_map(map_path("synthetic64.txt"))), E, A, P, T, seed=7, tracker="fresh",
                              shaping="qmix", max_other_robots=15, max_packages_obs=20, max_robots_state=16,
                              max_packages_state=100)
    gen = torch.Generator(device=dev).manual_seed(0)
    w = torch.randn(env.actor_vec_dim, 15, device=dev, generator=gen)
    h0 = torch.zeros(1, 4, device=dev)

    class Agent:
        def init_hidden(self):
            return h0

        def __call__(self, so, vo, h):
            return vo @ w, h

    ag = Agent()
    out = {}
    for name, dt in (("float32", torch.float32), ("bfloat16", torch.bfloat16)):
        col = QmixCollector(env, T, seed=1, ego_radius=R, ego_dtype=dt)
        col.collect(ag, 0.05, graph=True)   # eager, then the capture
        n = max(2, steps // 100)
        times = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                col.collect(ag, 0.05, graph=True)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) / n)
        out[name] = {"ms_per_collect": [x * 1e3 for x in times],
                     "us_per_env_step": [x * 1e6 / (E * col.L) for x in times],
                     "us_per_step": [x * 1e6 / col.L for x in times],
                     "so_bytes": col.so.numel() * col.so.element_size(),
                     "mean_episode_length": float(col.episode_length.double().mean())}
        del col
    print(json.dumps({"config": "5:ego_collect", "envs": E, "agents": A, "packages": P, "map": [64, 64], "radius": R,
                      "L": T, "collects_per_round": n, "rounds": 3, "collect": out}), flush=True)
    env.close()


def run_canvas(cfg, canvas, steps, warmup, rounds=3):
    """The critic map on a fixed canvas ("Canvas critic maps").

    Config 3 or 5: in one process, on one engine, ``build_obs_canvas(canvas, which=("critic_map",))`` over all
    of the rank's envs in one call, at the map's own shape (the identity) and at ``canvas``, float32 and
    bfloat16, beside the existing ``build_obs(which=("critic_map",))`` (float32; config 5: per chunk of 4,096
    envs, as its usual leg builds them).  Every figure is a hipGraph of 10 captured calls, each graph captured
    once and replayed in turn, ``rounds`` times -- the builds alternate inside one session.

    Config 4: a graphed ``MappoRollout(ego_radius=5, canvas=canvas)`` on its map mix (map1 .. map5) at 4,096
    envs, per env-step, beside the single-shape ego rollout of the same size on map1."""
    import marl_gpu
    from marl_gpu.maps import grid_array, load_map, map_path
    dev = torch.device("cuda", 0)
    Hc, Wc = canvas
    if cfg == "4":
        import marl_gpu.rollout as R
        E, A, P, T, Tr = 4096, 5, 50, 500, 64
        maps = [grid_array(load_map(map_path(f"map{i}.txt"))) for i in range(1, 6)]
        sizes = [E // 5 + (1 if i < E % 5 else 0) for i in range(5)]
        env_map = np.concatenate([np.full(s, i) for i, s in enumerate(sizes)])
        mixed = marl_gpu.BatchedEnv(maps, E, A, P, T, seed=42, env_map=env_map, tracker="mappo", max_packages_obs=5)
        single = marl_gpu.BatchedEnv(maps[0], E, A, P, T, seed=42, tracker="mappo", max_packages_obs=5)
        g = torch.Generator(device="cuda").manual_seed(0)
        wa = torch.randn(mixed.actor_vec_dim, 15, device="cuda", generator=g) * 0.1
        wc = torch.randn(mixed.critic_vec_dim, device="cuda", generator=g) * 0.01
        actor = lambda obs, vec: vec @ wa  # noqa: E731
        critic = lambda gmap, gvec: gvec @ wc  # noqa: E731
        legs = {"mixed_canvas": R.MappoRollout(mixed, Tr, seed=1, ego_radius=5, canvas=canvas),
                "single_shape_ego": R.MappoRollout(single, Tr, seed=1, ego_radius=5)}
        for env in (mixed, single):
            env.reset()
        for ro in legs.values():
            ro.collect(actor, critic, graph=True)   # runs eagerly and captures
        n = max(1, steps // Tr)
        t = {k: [] for k in legs}
        for _ in range(rounds):
            for k, ro in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(n):
                    ro.collect(actor, critic, graph=True)
                torch.cuda.synchronize()
                t[k].append((time.perf_counter() - t0) / (n * Tr) * 1e6)
        print(json.dumps({"config": "4:canvas_rollout", "envs": E, "agents": A, "packages": P, "canvas": [Hc, Wc],
                          "maps": [list(m.shape) for m in maps], "ego_radius": 5, "rollout_steps": Tr, "rollouts": n,
                          "rounds": rounds, "us_per_env_step": t}), flush=True)
        mixed.close()
        single.close()
        return
    if cfg == "3":
        E, A, P, T, H = 16384, 5, 50, 500, 10
        env = marl_gpu.BatchedEnv(grid_array(load_map(map_path("map1.txt"))), E, A, P, T, seed=42, tracker="mappo",
                                  max_other_robots=4, max_packages_obs=5)
        chunk = E
    elif cfg == "5":
        E, A, P, T, H = 131072 // 8, 16, 100, 500, 64
        env = marl_gpu.BatchedEnv(grid_array(load_map(map_path("synthetic64.txt"))), E, A, P, T, seed=7,
                                  tracker="mappo", max_other_robots=15, max_packages_obs=20, max_robots_state=16,
                                  max_packages_state=100)
        chunk = int(os.environ.get("MDL_OBS_CHUNK", "4096"))
    else:
        raise SystemExit("--canvas goes with --config 3, 4 or 5")
    env.reset()
    gen = torch.Generator(device=dev).manual_seed(0)
    G, C = 50, 10
    acts = torch.randint(0, 15, (G, E, A), generator=gen, device=dev, dtype=torch.int32).to(torch.uint8)
    for k in range(warmup):
        env.step(acts[k % G])
    nchunks = E // chunk
    full = {"critic_map": torch.empty((chunk, 4, H, H), dtype=torch.float32, device=dev)}

    def full_():
        for k in range(C):
            env.build_obs((k % nchunks) * chunk, chunk, out=full, which=("critic_map",))

    graphs = {"build_obs_float32": (_graph_of(full_), full, chunk * 4 * H * H * 4)}
    for cv in dict.fromkeys(((H, H), (Hc, Wc))):
        for n in ("float32", "bfloat16"):
            buf = {"critic_map": torch.empty((E, 4) + cv, dtype=OBS_DTYPES[n], device=dev)}

            def canvas_(buf=buf, cv=cv, n=n):
                for k in range(C):
                    env.build_obs_canvas(cv, out=buf, which=("critic_map",), dtype=OBS_DTYPES[n])

            graphs[f"canvas_{cv[0]}x{cv[1]}_{n}"] = (_graph_of(canvas_), buf,
                                                    buf["critic_map"].numel() * buf["critic_map"].element_size())
    reps = max(1, steps // 50)
    t = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, (g, _, _) in graphs.items():
            t[k].append(_replay_us(g, reps, C))
    res = {}
    for k, (_, _, b) in graphs.items():
        best = min(t[k])
        res[k] = {"us_per_call": t[k], "envs_per_call": chunk if k.startswith("build_obs") else E, "bytes_written": b,
                  "achieved_GBs": b / (best * 1e-6) / 1e9, "frac_of_8TBs": b / (best * 1e-6) / 1e9 / HBM}
    res["build_obs_float32"]["us_all_envs"] = [x * nchunks for x in t["build_obs_float32"]]
    print(json.dumps({"config": cfg + ":canvas", "envs": E, "agents": A, "packages": P, "map": [H, H],
                      "canvas": [Hc, Wc], "rounds": rounds, "replays": reps, "calls_per_graph": C, "builds": res}),
          flush=True)
    env.close()


def run_rollout(steps, graph=False, obs_dtype="float32"):
    """MAPPO rollout on the device: 4096 envs, map1, A=5, the
    trainer's featurizer sizes, a linear actor on the 52-dim vector and a linear
    critic on the 1301-dim vector; sampling, step, obs into the buffers and GAE
    all on the device.  Reports env agent-steps/s of whole rollouts."""
    import marl_gpu
    import marl_gpu.rollout as R
    from marl_gpu.maps import grid_array, load_map, map_path
    E, A, P, T = 4096, 5, 50, 500
    env = marl_gpu.BatchedEnv(grid_array(load_map(map_path("map1.txt"))), E, A, P, T, seed=42, tracker="mappo",
                              max_other_robots=A - 1, max_packages_obs=5)
    env.reset()
    g = torch.Generator(device="cuda").manual_seed(0)
    wa = torch.randn(env.actor_vec_dim, 15, device="cuda", generator=g) * 0.1
    wc = torch.randn(env.critic_vec_dim, device="cuda", generator=g) * 0.01
    actor = lambda obs, vec: vec.float() @ wa  # noqa: E731  (float(): the identity on float32 observations)
    critic = lambda gmap, gvec: gvec.float() @ wc  # noqa: E731
    Tr = 128
    ro = R.MappoRollout(env, Tr, seed=1) if obs_dtype == "float32" \
        else R.MappoRollout(env, Tr, seed=1, obs_dtype=OBS_DTYPES[obs_dtype])
    ro.collect(actor, critic, graph=graph)   # (graph: this call runs eagerly and captures)
    torch.cuda.synchronize()
    n = max(1, steps // Tr)
    t0 = time.perf_counter()
    for _ in range(n):
        ro.collect(actor, critic, graph=graph)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out = {"config": "rollout_graph" if graph else "rollout", "envs": E, "agents": A, "rollout_steps": Tr, "rollouts": n,
           "obs_dtype": obs_dtype,
           "us_per_env_step": dt / (n * Tr) * 1e6, "agent_steps_per_s": E * A * n * Tr / dt,
           "note": "MappoRollout.collect: linear actor/critic (torch), on-device sampling, mdl_step_obs (step + "
                   "next observations in one launch) into the rollout buffers, GAE kernel"}
    print(json.dumps(out))


def run_alt(steps):
    """IDQ/qmix featurizers on 4096 map1 envs, A=5: convert_state for every
    agent (6 x H x W) and convert_global_state_to_tensor (7 x H x W), written by one kernel."""
    import marl_gpu
    from marl_gpu.maps import grid_array, load_map, map_path
    E, A, P, T, H, W = 4096, 5, 50, 500, 10, 10
    env = marl_gpu.BatchedEnv(grid_array(load_map(map_path("map1.txt"))), E, A, P, T, seed=42, tracker="fresh")
    env.reset()
    gen = torch.Generator(device="cuda").manual_seed(0)
    for k in range(60):
        env.step(torch.randint(0, 15, (E, A), generator=gen, device="cuda", dtype=torch.int32).to(torch.uint8))
    out = env.build_obs_alt()
    us = timed(lambda k: env.build_obs_alt(out=out), max(20, steps // 5))
    nbytes = E * 4 * (A * 6 * H * W + 7 * H * W)
    print(json.dumps({"config": "alt_featurizers", "envs": E, "agents": A, "us_per_call": us, "write_bytes": nbytes,
                      "roofline": {"achieved_GBs": nbytes / (us * 1e-6) / 1e9, "frac": nbytes / (us * 1e-6) / 1e9 / HBM},
                      "note": "mdl_build_obs_alt: IDQ convert_state x A + qmix convert_global_state_to_tensor"}),
          flush=True)
    env.close()


def run_greedy(steps):
    """Batched greedy baseline: 4096 map1 envs, A=5, one greedyagent.py
    get_actions per env plus the step, per env-step (one episode, no resets)."""
    import marl_gpu
    from marl_gpu.maps import grid_array, load_map, map_path
    E, A, P, T = 4096, 5, 50, 500
    env = marl_gpu.BatchedEnv(grid_array(load_map(map_path("map1.txt"))), E, A, P, T, seed=42, tracker="fresh")
    env.reset()
    env.greedy_init()
    acts = torch.empty((E, A), dtype=torch.uint8, device="cuda")
    n = min(steps, T - 20)

    def one(k):
        env.greedy_actions(out=acts)
        env.step(acts, auto_reset=False, action_format="codes")

    for k in range(10):
        one(k)
    us = timed(one, n)
    g_us = timed(lambda k: env.greedy_actions(out=acts), 20)
    print(json.dumps({"config": "greedy", "envs": E, "agents": A, "us_per_env_step": us,
                      "agent_steps_per_s": E * A / (us * 1e-6), "greedy_actions_us": g_us,
                      "note": "greedy_actions (BFS distance tables precomputed per map) + mdl_step per env-step"}),
          flush=True)
    env.close()


def _graph_of(fn):
    """fn() captured once as a hipGraph (after one eager call)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        fn()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            fn()
    torch.cuda.synchronize()
    return g


def _replay_us(g, reps, per):
    g.replay()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / (reps * per) * 1e3


def run_qmix(steps):
    """QMIX episode collection ("QMIX episode collection").

    1. The masked step against the full step: ``step_episode`` with every env active against
       ``step_obs(auto_reset=False)`` on the same engine in the same run, hipGraph-replayed, five
       repeats each, interleaved.  Both graphs are [reset, mask fill, G steps], so no env ends inside
       one and the fixed part is the same on both sides.  map1, A=5, P=20; 16,384 envs and 4.
    2. One collector step (``select_actions_eps`` + ``step_episode``, half of the envs inactive)
       against the host-driven subset loop it replaces (done mask read back, id list built on the
       host and uploaded, action rows gathered, ``step(env_ids=...)``, ``build_obs()``); 4 and 4,096 envs.
    """
    import marl_gpu
    import marl_gpu.qmix_rollout as Q
    from marl_gpu.maps import grid_array, load_map, map_path
    g1 = grid_array(load_map(map_path("map1.txt")))
    A, P, T, G = 5, 20, 500, 50
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    reps = max(2, steps // G)
    for E in (16384, 4):
        env = marl_gpu.BatchedEnv(g1, E, A, P, T, seed=42, tracker="fresh", shaping="qmix")
        acts = torch.randint(0, 15, (G, E, A), generator=gen, device=dev, dtype=torch.int32).to(torch.uint8)
        bufs = env.obs_buffers()
        out = (torch.zeros(E, dtype=torch.float64, device=dev), torch.zeros(E, dtype=torch.float32, device=dev),
               torch.zeros(E, dtype=torch.uint8, device=dev))
        active = torch.ones(E, dtype=torch.uint8, device=dev)
        filled = torch.zeros(E, dtype=torch.uint8, device=dev)

        def full():
            env.reset()
            active.fill_(1)
            for k in range(G):
                env.step_obs(acts[k], auto_reset=False, out=out, obs_out=bufs)

        def masked():
            env.reset()
            active.fill_(1)
            for k in range(G):
                env.step_episode(acts[k], active, out=out, filled=filled, obs_out=bufs)

        gf, gm = _graph_of(full), _graph_of(masked)
        tf, tm = [], []
        for _ in range(5):
            tf.append(_replay_us(gf, reps, G))
            tm.append(_replay_us(gm, reps, G))
        assert bool(active.all()), "an env ended inside the measured graph"
        print(json.dumps({"config": "qmix_masked_step", "envs": E, "agents": A, "packages": P, "graph_steps": G,
                          "replays": reps, "step_obs_us": tf, "step_episode_us": tm,
                          "step_obs_spread_us": max(tf) - min(tf), "median_gap_us": float(np.median(tm) - np.median(tf)),
                          "kernels": [env.step_kernel_name(with_obs=True), "mdl::k_step_episode (same shapes)"],
                          "note": "us per step of [reset, mask fill, 50 steps] graphs, every env active"}), flush=True)
        env.close()

    for E in (4, 4096):
        env = marl_gpu.BatchedEnv(g1, E, A, P, T, seed=42, tracker="fresh", shaping="qmix")
        ref = marl_gpu.BatchedEnv(g1, E, A, P, T, seed=42, tracker="fresh", shaping="qmix")
        q = torch.randn(G, E * A, 15, generator=gen, device=dev)
        half = (torch.arange(E, device=dev) % 2 == 0).to(torch.uint8)
        u = torch.zeros((E, A), dtype=torch.uint8, device=dev)
        bufs = env.obs_buffers()
        out = (torch.zeros(E, dtype=torch.float64, device=dev), torch.zeros(E, dtype=torch.float32, device=dev),
               torch.zeros(E, dtype=torch.uint8, device=dev))
        active = torch.ones(E, dtype=torch.uint8, device=dev)
        filled = torch.zeros(E, dtype=torch.uint8, device=dev)

        def coll_step(k):
            Q.select_actions_eps(q[k % G], 0.2, 1, k, out=u.view(-1))
            env.step_episode(u, active, out=out, filled=filled, obs_out=bufs)

        def coll_graph():
            env.reset()
            active.copy_(half)
            for k in range(G):
                coll_step(k)

        env.reset()
        active.copy_(half)
        for k in range(5):
            coll_step(k)
        env.reset()
        active.copy_(half)
        coll_eager = timed(coll_step, G)
        coll_g = _replay_us(_graph_of(coll_graph), reps, G)

        rbufs = ref.obs_buffers()
        state = {"done": torch.zeros(E, dtype=torch.uint8, device=dev), "mask": half.cpu().numpy().astype(bool)}

        def host_step(k):
            # the parent's path (tests/test_gpu_parity.py::test_qmix_rollout_golden): one round trip to
            # learn which envs finished, a host-built id list, the subset step, the observation build
            state["mask"] &= ~state["done"].cpu().numpy().astype(bool)
            idx = np.nonzero(state["mask"])[0]
            ids = torch.from_numpy(idx.astype(np.int32)).to(dev)
            a = q[k % G].view(E, A, 15)[:, :, 0].gt(0).to(torch.uint8)[ids.long()].contiguous()   # stand-in actions
            _, _, dn = ref.step(a, env_ids=ids, auto_reset=False)
            state["done"].zero_()
            state["done"][ids.long()] = dn
            ref.build_obs(out=rbufs)

        ref.reset()
        for k in range(5):   # torch's indexing kernels and the copy paths, once
            host_step(k)
        ref.reset()
        state["done"].zero_()
        state["mask"] = half.cpu().numpy().astype(bool)
        host_us = timed(host_step, G)
        print(json.dumps({"config": "qmix_collector_step", "envs": E, "agents": A, "active_fraction": 0.5,
                          "collector_step_graph_us": coll_g, "collector_step_eager_us": coll_eager,
                          "host_loop_step_us": host_us,
                          "launches": {"collector": "2 kernels (k_select_eps, k_step_episode), no copy, no sync",
                                       "host_loop": "k_step (subset) + k_obs_small + the torch gather/scatter kernels, "
                                                    "1 D2H + 1 H2D copy, 1 host sync per step"}}), flush=True)
        env.close()
        ref.close()


def _pack_idq_views(s0, s1, idx, A, P):
    """Host side of mdl_views_idq_reward for the envs ``idx``: the previous states with their
    trackers as view records of fixed width, the current robot records, the offsets (numpy)."""
    n = idx.size
    vw, cw = 4 + 3 * A + 8 * P, 2 + 3 * A
    trk, data = s0["tracker"][idx], s0["tracker_data"][idx]
    pres = trk[:, :, 0] != 0
    order = np.argsort(~pres, axis=1, kind="stable")                 # present slots first
    rows = np.zeros((n, P, 8), np.int32)
    rows[:, :, 0] = order + 1
    rows[:, :, 1] = np.where(np.take_along_axis(trk[:, :, 1], order, 1) != 0, 2, 1)
    rows[:, :, 2:] = np.take_along_axis(data, order[:, :, None], 1)
    views = np.zeros((n, vw), np.int32)
    views[:, 0] = s0["t"][idx]
    views[:, 1] = A
    views[:, 2] = pres.sum(1)
    views[:, 4:4 + 3 * A] = s0["robots"][idx].reshape(n, 3 * A)
    views[:, 4 + 3 * A:] = rows.reshape(n, 8 * P)
    cur = np.zeros((n, cw), np.int32)
    cur[:, 0] = s1["t"][idx]
    cur[:, 1] = A
    cur[:, 2:] = s1["robots"][idx].reshape(n, 3 * A)
    ar = np.arange(n, dtype=np.int64)
    return views, cur, ar * vw, ar * cw, ar * A


def run_idq(steps):
    """IDQ transition collection ("IDQ transition collection"); map1, A=5, P=20, fresh
    tracker, 4 and 4,096 envs, every env running.

    1. ``alt_transition`` alone against ``build_obs_alt`` alone on the same envs and state
       (idq_obs only), hipGraph-replayed, five repeats each, interleaved: the cost of the row mask,
       the reward and the pre-record.
    2. One ``IdqCollector`` step (selection, ``step_episode``, ``alt_transition``, the replay
       append; the agent's forward replaced by preset Q-values), eager and graph-replayed, against
       the host-driven loop the engine allowed before, five interleaved repeats: done mask read
       back, subset ``step``, ``read_state`` before and after the step, views packed on the host
       and uploaded, ``mdl_views_idq_reward``, ``build_obs_alt``, torch indexed ring writes.
    """
    import marl_gpu
    from marl_gpu._lib import check, lib, ptr, stream_handle
    from marl_gpu.idq_rollout import IdqCollector, TransitionReplay
    from marl_gpu.maps import grid_array, load_map, map_path
    g1 = grid_array(load_map(map_path("map1.txt")))
    H, W = g1.shape
    A, P, T, G = 5, 20, 500, 50
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    reps = max(2, steps // G)
    for E in (4, 4096):
        env = marl_gpu.BatchedEnv(g1, E, A, P, T, seed=42, tracker="fresh")
        env.reset()
        acts = torch.randint(0, 15, (E, A), generator=gen, device=dev, dtype=torch.int32).to(torch.uint8)
        for _ in range(30):
            env.step(acts, auto_reset=False)
        obs = {"idq_obs": torch.zeros((E, A, 6, H, W), dtype=torch.float32, device=dev)}
        pre = env.alt_pre_buffer()
        ones = torch.ones(E, dtype=torch.uint8, device=dev)
        r = torch.zeros((E, A), dtype=torch.float64, device=dev)
        env.alt_transition(None, pre, out=obs)

        def many(fn):
            def f():
                for _ in range(G):
                    fn()
            return f

        gb = _graph_of(many(lambda: env.build_obs_alt(out=obs, which=("idq_obs",))))
        gt = _graph_of(many(lambda: env.alt_transition(acts, pre, ops_are_ints=True, out=obs, r_out=r)))
        gm = _graph_of(many(lambda: env.alt_transition(acts, pre, row_mask=ones, ops_are_ints=True, out=obs, r_out=r)))
        tb, tt, tm = [], [], []
        for _ in range(5):
            tb.append(_replay_us(gb, reps, G))
            tt.append(_replay_us(gt, reps, G))
            tm.append(_replay_us(gm, reps, G))
        print(json.dumps({"config": "idq_alt_transition", "envs": E, "agents": A, "packages": P, "graph_calls": G,
                          "replays": reps, "build_obs_alt_us": tb, "alt_transition_us": tt,
                          "alt_transition_masked_us": tm, "build_obs_alt_spread_us": max(tb) - min(tb),
                          "median_gap_us": float(np.median(tt) - np.median(tb)),
                          "median_gap_masked_us": float(np.median(tm) - np.median(tb)),
                          "note": "us per call, idq_obs only, same envs and state; masked = row_mask all ones"}),
              flush=True)
        env.close()

    for E in (4, 4096):
        cap = 1 << 16
        env = marl_gpu.BatchedEnv(g1, E, A, P, T, seed=42, tracker="fresh")
        ref = marl_gpu.BatchedEnv(g1, E, A, P, T, seed=42, tracker="fresh")
        q = torch.randn(E * A, 15, generator=gen, device=dev)
        agent = lambda o: q   # noqa: E731  (stand-in for the network's forward)
        col = IdqCollector(env, TransitionReplay(cap, (6, H, W), device=dev), seed=1, ops_are_ints=True)

        # the host-driven loop
        ring = TransitionReplay(cap, (6, H, W), device=dev)   # only its tensors: written by torch indexing
        o2 = [torch.zeros((E, A, 6, H, W), dtype=torch.float32, device=dev) for _ in range(2)]
        st = {"done": torch.zeros(E, dtype=torch.uint8, device=dev), "mask": np.ones(E, bool), "ptr": 0, "cur": 0}
        a_all = q.view(E, A, 15)[:, :, 0].gt(0).to(torch.uint8)   # stand-in actions

        def host_step(k):
            st["mask"] &= ~st["done"].cpu().numpy().astype(bool)                      # done mask read back
            idx = np.nonzero(st["mask"])[0]
            n = idx.size
            ids = torch.from_numpy(idx.astype(np.int32)).to(dev)
            il = ids.long()
            a = a_all[il].contiguous()
            s0 = {k2: v.cpu().numpy() for k2, v in ref.read_state().items()}           # state before the step
            _, _, dn = ref.step(a, env_ids=ids, auto_reset=False)
            st["done"].zero_()
            st["done"][il] = dn
            s1 = {k2: v.cpu().numpy() for k2, v in ref.read_state().items()}           # and after it
            views, cur, vo, co, oo = _pack_idq_views(s0, s1, idx, A, P)
            dv, dc = torch.from_numpy(views).to(dev), torch.from_numpy(cur).to(dev)
            dvo, dco, doo = (torch.from_numpy(x).to(dev) for x in (vo, co, oo))
            rw = torch.empty(n * A, dtype=torch.float64, device=dev)
            check(lib().mdl_views_idq_reward(ref._h, ptr(dv), ptr(dvo), P, ptr(dc), ptr(dco), ptr(a), ptr(doo), 1, n,
                                             ptr(rw), stream_handle(dev)), "mdl_views_idq_reward")
            c = st["cur"]
            ref.build_obs_alt(out={"idq_obs": o2[1 - c]}, which=("idq_obs",))
            slots = (torch.arange(n * A, device=dev) + st["ptr"]) % cap                # the ring writes
            ring.observations[slots] = o2[c][il].reshape(n * A, 6, H, W)
            ring.next_observations[slots] = o2[1 - c][il].reshape(n * A, 6, H, W)
            ring.actions[slots] = a.reshape(-1).long()
            ring.rewards[slots] = rw.float()
            ring.dones[slots] = dn.repeat_interleave(A)
            st["ptr"] = (st["ptr"] + n * A) % cap
            st["cur"] = 1 - c

        def host_begin():
            ref.reset()
            st["done"].zero_()
            st["mask"][:] = True
            st["cur"] = 0
            ref.build_obs_alt(out={"idq_obs": o2[0]}, which=("idq_obs",))

        host_begin()
        for k in range(5):   # torch's indexing kernels and the copy paths, once
            host_step(k)
        col.begin()
        for k in range(5):
            col.step(agent, 0.2)
        col.collect(agent, 0.2, max_steps=G, graph=True)   # eager run + capture
        te, tg, th = [], [], []
        for _ in range(5):
            col.begin()
            te.append(timed(lambda k: col.step(agent, 0.2), G))
            tg.append(timed(lambda k: col.collect(agent, 0.2, max_steps=G, graph=True), reps) / G)
            host_begin()
            th.append(timed(host_step, G))
        assert col.captured_graphs() == {None: G} and bool(col.active.all()), "an env ended inside the measured collect"
        print(json.dumps({"config": "idq_collector_step", "envs": E, "agents": A, "packages": P, "steps": G,
                          "collector_step_graph_us": tg, "collector_step_eager_us": te, "host_loop_step_us": th,
                          "graph_spread_us": max(tg) - min(tg), "eager_spread_us": max(te) - min(te),
                          "host_spread_us": max(th) - min(th),
                          "launches": {"collector": "5 kernels (k_select_eps, k_step_episode, k_alt_transition, "
                                                    "k_replay_rank, k_replay_copy), no copy, no sync; the graph figure "
                                                    "holds 1/50 of the collect's reset, begin and return read",
                                       "host_loop": "k_step (subset), 2 k_export, k_views_idq_reward, k_alt_obs, the torch "
                                                    "gather/scatter kernels, 13 D2H + 6 H2D copies per step"}}),
              flush=True)
        env.close()
        ref.close()


def run_qmix_cycle(steps):
    """map-QMIX cycle collection ("map-QMIX cycle collection"); map1, A=5, P=20, fresh
    tracker, 4 and 4,096 envs, T = 50 with the episodes staggered by initial marks (env e is marked
    at warm-up step e % T), so the resets spread over the steps.  hipGraphs of G calls, five
    interleaved repeats each.

    1. ``cycle_begin`` with an all-zero mask; ``cycle_begin`` with every env marked against
       ``reset`` + ``build_obs_alt`` as two launches (both behind the same ``fill_`` of the mask).
    2. ``JointReplay.add`` alone, with the bytes it moves (from the shapes) and GB/s.
    3. One ``QmixCycleCollector`` step (the agent's forward replaced by preset Q-values), eager
       and graph-replayed, against the host-driven loop it replaces: done flags read back, the id
       list built on the host, ``clear_tracker`` / ``reset(ids)``, ``build_obs_alt``, torch index
       copies into a ring.
    """
    import marl_gpu
    from marl_gpu.maps import grid_array, load_map, map_path
    from marl_gpu.qmix_cycle import JointReplay, QmixCycleCollector
    g1 = grid_array(load_map(map_path("map1.txt")))
    H, W = g1.shape
    A, P, T, G, cap = 5, 20, 50, 50, 8192
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    reps = max(2, steps // G)

    def many(fn):
        def f():
            for _ in range(G):
                fn()
        return f

    for E in (4, 4096):
        env = marl_gpu.BatchedEnv(g1, E, A, P, T, seed=42, tracker="fresh")
        ref = marl_gpu.BatchedEnv(g1, E, A, P, T, seed=42, tracker="fresh")
        q = torch.randn(E * A, 15, generator=gen, device=dev)
        agent = lambda o: q   # noqa: E731  (stand-in for the network's forward)
        rep = JointReplay(cap, A, (6, H, W), (7, H, W), device=dev)
        col = QmixCycleCollector(env, rep, seed=1)
        col.begin()
        for k in range(T):                              # stagger the episodes
            col.done[k::T] = 1
            col.step(agent, 0.2)

        # 1. cycle_begin alone (on `ref`, which the collector does not use)
        ref.reset()
        out = {"idq_obs": torch.zeros((E, A, 6, H, W), dtype=torch.float32, device=dev),
               "qmix_state": torch.zeros((E, 7, H, W), dtype=torch.float32, device=dev)}
        mask = torch.zeros(E, dtype=torch.uint8, device=dev)
        comp = torch.zeros(E, dtype=torch.uint8, device=dev)
        cret = torch.zeros(E, dtype=torch.float64, device=dev)
        cst = torch.zeros(E, dtype=torch.int32, device=dev)

        def begin_zero():
            ref.cycle_begin(mask, out=out, completed=comp, completed_return=cret, completed_steps=cst)

        def begin_all():
            mask.fill_(1)
            ref.cycle_begin(mask, out=out, completed=comp, completed_return=cret, completed_steps=cst)

        def two_launches():
            mask.fill_(1)
            ref.reset()
            ref.build_obs_alt(out=out)

        gz, ga, g2 = _graph_of(many(begin_zero)), _graph_of(many(begin_all)), _graph_of(many(two_launches))
        tz, ta, t2 = [], [], []
        for _ in range(5):
            tz.append(_replay_us(gz, reps, G))
            ta.append(_replay_us(ga, reps, G))
            t2.append(_replay_us(g2, reps, G))
        print(json.dumps({"config": "qmix_cycle_begin", "envs": E, "agents": A, "packages": P, "graph_calls": G,
                          "replays": reps, "cycle_begin_zero_mask_us": tz, "cycle_begin_all_marked_us": ta,
                          "reset_plus_build_obs_alt_us": t2,
                          "note": "us per call; the marked and the two-launch figures include one fill_ of the mask"}),
              flush=True)

        # 2. the append alone
        # Four source sets taken in turn and a ring of 16 steps: at 4,096 envs a step reads 121 MB and
        # writes 121 MB, so neither the sources (485 MB) nor the ring (1.9 GB) fit the 256 MB
        # Infinity Cache and the GB/s figure is HBM traffic.
        NS, cap2 = 4, 16 * max(E, 4)
        f32 = dict(dtype=torch.float32, device=dev)
        src = [(torch.zeros((E, 7, H, W), **f32), torch.zeros((E, 7, H, W), **f32),
                torch.zeros((E, A, 6, H, W), **f32), torch.zeros((E, A, 6, H, W), **f32)) for _ in range(NS)]
        u = torch.zeros((E, A), dtype=torch.uint8, device=dev)
        rw = torch.zeros(E, dtype=torch.float64, device=dev)
        dn = torch.zeros(E, dtype=torch.uint8, device=dev)
        ring2 = JointReplay(cap2, A, (6, H, W), (7, H, W), device=dev)

        def adds():
            for k in range(G):
                s1, s2, o1, o2 = src[k % NS]
                ring2.add(s1, s2, o1, o2, u, rw, dn)

        gadd = _graph_of(adds)
        tadd = [_replay_us(gadd, reps, G) for _ in range(5)]
        row = 2 * (7 * H * W + A * 6 * H * W) * 4
        moved = E * (2 * row + A * (1 + 8) + (8 + 4) + (1 + 1))        # read + written, from the shapes
        print(json.dumps({"config": "qmix_joint_add", "envs": E, "agents": A, "capacity": cap2, "source_sets": NS,
                          "graph_calls": G, "replays": reps, "add_us": tadd, "bytes_moved": moved,
                          "gb_per_s": [moved / (t * 1e-6) / 1e9 for t in tadd]}), flush=True)
        del ring2, gadd, src

        # 3. one collector step against the host-driven loop
        ring = JointReplay(cap, A, (6, H, W), (7, H, W), device=dev)   # only its tensors: written by torch indexing
        ob = [torch.zeros((E, A, 6, H, W), dtype=torch.float32, device=dev) for _ in range(2)]
        sb = [torch.zeros((E, 7, H, W), dtype=torch.float32, device=dev) for _ in range(2)]
        st = {"done": torch.zeros(E, dtype=torch.uint8, device=dev), "ptr": 0, "cur": 0}
        r_env = torch.zeros(E, dtype=torch.float64, device=dev)
        r_sh = torch.zeros(E, dtype=torch.float32, device=dev)
        a_all = q.view(E, A, 15)[:, :, 0].gt(0).to(torch.uint8).contiguous()   # stand-in actions
        ar = torch.arange(E, device=dev)

        def host_step(k):
            c = st["cur"]
            idx = np.nonzero(st["done"].cpu().numpy())[0]                              # done flags read back
            if idx.size:
                ref.clear_tracker(idx)
                ref.reset(idx)
                ref.build_obs_alt(out={"idq_obs": ob[c], "qmix_state": sb[c]})        # the reset rows (all rebuilt)
            ref.step(a_all, auto_reset=False, out=(r_env, r_sh, st["done"]))
            ref.build_obs_alt(out={"idq_obs": ob[1 - c], "qmix_state": sb[1 - c]})
            slots = (ar + st["ptr"]) % cap                                             # the ring writes
            ring.states[slots] = sb[c]
            ring.next_states[slots] = sb[1 - c]
            ring.observations[slots] = ob[c]
            ring.next_observations[slots] = ob[1 - c]
            ring.actions[slots] = a_all.long()
            ring.total_reward[slots, 0] = r_env.float()
            ring.dones[slots, 0] = st["done"]
            st["ptr"] = (st["ptr"] + E) % cap
            st["cur"] = 1 - c

        ref.reset()
        ref.build_obs_alt(out={"idq_obs": ob[0], "qmix_state": sb[0]})
        for k in range(T):                              # the same stagger, and torch's indexing kernels once
            st["done"][k::T] = 1
            host_step(k)
        col.cycle(agent, 0.2, G, graph=True)            # eager run + capture
        col.cycle(agent, 0.2, G, graph=True)
        te, tg, th = [], [], []
        for _ in range(5):
            te.append(timed(lambda k: col.step(agent, 0.2), G))
            tg.append(timed(lambda k: col.cycle(agent, 0.2, G, graph=True), reps) / G)
            th.append(timed(host_step, G))
        assert len(col.captured_graphs()) >= 1
        print(json.dumps({"config": "qmix_cycle_step", "envs": E, "agents": A, "packages": P, "steps": G,
                          "max_time_steps": T, "collector_step_graph_us": tg, "collector_step_eager_us": te,
                          "host_loop_step_us": th,
                          "launches": {"collector": "k_cycle_begin, k_select_eps, k_step, k_alt_obs, k_replay_copy_joint, "
                                                    "k_replay_advance; no copy, no sync",
                                       "host_loop": "one D2H copy and sync per step, k_reset and k_alt_obs for the "
                                                    "reset envs, k_step, k_alt_obs, the torch scatter kernels"}}),
              flush=True)
        env.close()
        ref.close()


def run_eval_bench(steps):
    """Device-resident evaluation ("Evaluation"); the README configuration (map1, A=5,
    P=100, T=1000, fresh tracker, env e seeded 10 + e) at 100 and 4,096 envs.  hipGraphs of G calls,
    five interleaved repeats each.

    1. ``greedy_actions()`` against ``greedy_actions_masked`` with an all-ones and with an all-zero
       mask, 30 steps into the episodes.  get_actions appends this t's spawns to the agent record on
       every call, so each graph is [greedy_init, G calls]: every replay starts from the same record
       (the all-zero side carries the same greedy_init).
    2. ``episode_results`` against the ``mdl_read_state`` export it replaces (all six tables, into
       preallocated tensors: the allocations ``read_state`` makes are left out).
    3. One whole greedy evaluation -- reset, greedy_init, T x [actions, step], results, one
       synchronisation -- by the ``Evaluator`` graph-replayed and eager, against the host-driven loop
       of tests/test_gpu_greedy.py::run_greedy_episodes; wall time, and wall time / T per step.
    """
    import marl_gpu
    from marl_gpu._lib import check, lib, ptr, stream_handle
    from marl_gpu.maps import grid_array, load_map, map_path
    g1 = grid_array(load_map(map_path("map1.txt")))
    A, P, T, G = 5, 100, 1000, 50
    dev = torch.device("cuda", 0)
    reps = max(2, steps // G)

    def wall_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for E in (100, 4096):
        seeds = [10 + e for e in range(E)]
        env = marl_gpu.BatchedEnv(g1, E, A, P, T, seeds=seeds, tracker="fresh")
        env.reset()
        env.greedy_init()
        acts = torch.zeros((E, A), dtype=torch.uint8, device=dev)
        ones = torch.ones(E, dtype=torch.uint8, device=dev)
        zeros = torch.zeros(E, dtype=torch.uint8, device=dev)
        for _ in range(30):
            env.greedy_actions(out=acts)
            env.step(acts, auto_reset=False, action_format="codes")

        # 1. the mask's cost
        def calls(fn):
            def f():
                env.greedy_init()
                for _ in range(G):
                    fn()
            return f

        gu = _graph_of(calls(lambda: env.greedy_actions(out=acts)))
        g1s = _graph_of(calls(lambda: env.greedy_actions_masked(ones, out=acts)))
        g0s = _graph_of(calls(lambda: env.greedy_actions_masked(zeros, out=acts)))
        tu, t1, t0 = [], [], []
        for _ in range(5):
            tu.append(_replay_us(gu, reps, G))
            t1.append(_replay_us(g1s, reps, G))
            t0.append(_replay_us(g0s, reps, G))
        print(json.dumps({"config": "eval_greedy_mask", "envs": E, "agents": A, "packages": P, "graph_calls": G,
                          "replays": reps, "greedy_actions_us": tu, "masked_all_ones_us": t1,
                          "masked_all_zero_us": t0,
                          "note": "us per call; every graph is [greedy_init, G calls], so each figure carries "
                                  "1/G of one greedy_init"}), flush=True)

        # 2. the results against the export
        i32 = dict(dtype=torch.int32, device=dev)
        res = (torch.zeros(E, dtype=torch.float64, device=dev), torch.zeros(E, **i32), torch.zeros(E, **i32))
        exp = dict(robots=torch.zeros((E, A, 3), **i32), pkgs=torch.zeros((E, P, 8), **i32), t=torch.zeros(E, **i32),
                   total=torch.zeros(E, dtype=torch.float64, device=dev), trk=torch.zeros((E, P, 4), **i32),
                   data=torch.zeros((E, P, 6), **i32))

        def export():
            check(lib().mdl_read_state(env._h, ptr(exp["robots"]), ptr(exp["pkgs"]), ptr(exp["t"]), ptr(exp["total"]),
                                       ptr(exp["trk"]), ptr(exp["data"]), stream_handle(dev)), "mdl_read_state")

        def many(fn):
            def f():
                for _ in range(G):
                    fn()
            return f

        gr, ge = _graph_of(many(lambda: env.episode_results(out=res))), _graph_of(many(export))
        tr, te = [], []
        for _ in range(5):
            tr.append(_replay_us(gr, reps, G))
            te.append(_replay_us(ge, reps, G))
        print(json.dumps({"config": "eval_results", "envs": E, "agents": A, "packages": P, "graph_calls": G,
                          "replays": reps, "episode_results_us": tr, "read_state_export_us": te,
                          "export_bytes": E * (A * 3 + P * 18 + 1 + 2) * 4, "results_bytes": E * 16}), flush=True)
        del gu, g1s, g0s, gr, ge

        # 3. one whole greedy evaluation
        ev = marl_gpu.Evaluator(env)
        got = {}

        def host_loop():
            env.reset()
            env.greedy_init()
            active = np.arange(E)
            totals, delivered = np.zeros(E), np.zeros(E, np.int64)
            while active.size:
                ids = torch.from_numpy(active.astype(np.int32)).cuda()
                a = env.greedy_actions(env_ids=ids)
                _, _, done = env.step(a, env_ids=ids, auto_reset=False, action_format="codes")
                d = done.cpu().numpy().astype(bool)
                if d.any():
                    s = env.read_state()
                    tot = s["total_reward"].cpu().numpy()
                    st = s["pkgs"][:, :, 7].cpu().numpy()
                    for e in active[d]:
                        totals[e] = tot[e]
                        delivered[e] = int((st[e] == 3).sum())
                    active = active[~d]
            got["host"] = (totals.tolist(), delivered.tolist())

        def evaluator(graph):
            def f():
                ev.run("greedy", graph=graph, graph_steps=G)
                s = ev.summary()
                got[graph] = (s["rewards"], s["delivered"])
            return f

        # every run resets the envs (their next layouts): rewound to the built engine before each
        # run, outside the timed region, all three play the README's episodes
        built = marl_gpu.BatchedEnv(g1, E, A, P, T, seeds=seeds, tracker="fresh")
        blob = built.save_state()
        built.close()

        def rewound(fn):
            env.load_state(blob)
            return wall_ms(fn)

        rewound(evaluator(True))                            # eager run + capture
        rewound(evaluator(True))
        rewound(host_loop)
        wg, we, wh = [], [], []
        for _ in range(5):
            wg.append(rewound(evaluator(True)))
            we.append(rewound(evaluator(False)))
            wh.append(rewound(host_loop))
        assert got[True] == got[False] == got["host"]
        print(json.dumps({"config": "eval_greedy_run", "envs": E, "agents": A, "packages": P, "max_time_steps": T,
                          "graph_steps": G, "evaluator_graph_ms": wg, "evaluator_eager_ms": we, "host_loop_ms": wh,
                          "evaluator_graph_step_us": [x * 1e3 / T for x in wg],
                          "evaluator_eager_step_us": [x * 1e3 / T for x in we],
                          "host_loop_step_us": [x * 1e3 / T for x in wh],
                          "mean_reward": float(np.mean(got[True][0])),
                          "launches": {"evaluator": "k_reset, k_greedy_init, T x (k_greedy_act, mdl_step_episode's launches), "
                                                    "k_episode_results; one copy and one sync at the end",
                                       "host_loop": "per step: the id list's upload, k_greedy_act, k_step, one D2H "
                                                    "copy and sync; k_export and two copies whenever an env ends"}}),
              flush=True)
        env.close()


def run_avail(steps, collect="both"):
    """The valid-action mask ("Valid-action masks").  hipGraphs of G calls, five
    interleaved repeats each.

    1. ``avail_actions`` per call with no mask, an all-ones and an all-zero ``active``, 30 greedy steps
       into the episodes of the README evaluation configuration (map1, A=5, P=100, T=1000, env e
       seeded 10 + e) at 100 and 4,096 envs, beside the existing launch-bound small kernels on the
       same box in the same run: ``episode_results`` and ``greedy_actions_masked`` with an all-zero
       mask (its graph is [greedy_init, G calls], as in --eval).
    2. ``QmixCollector.collect(graph=True)`` per env-step, L = 50, with ``avail`` on and off, a small
       GRU agent on the actor vector (map1, A=5, P=20, 100 and 4,096 envs).  collect="off" times the
       off case alone through the constructor without the argument.
    """
    import marl_gpu
    import marl_gpu.qmix_rollout as Q
    from marl_gpu.maps import grid_array, load_map, map_path
    g1 = grid_array(load_map(map_path("map1.txt")))
    dev = torch.device("cuda", 0)
    G = 50
    reps = max(2, steps // G)

    def many(fn):
        def f():
            for _ in range(G):
                fn()
        return f

    for E in (100, 4096) if collect == "both" else ():
        A, P, T = 5, 100, 1000
        env = marl_gpu.BatchedEnv(g1, E, A, P, T, seeds=[10 + e for e in range(E)], tracker="fresh")
        env.reset()
        env.greedy_init()
        acts = torch.zeros((E, A), dtype=torch.uint8, device=dev)
        ones = torch.ones(E, dtype=torch.uint8, device=dev)
        zeros = torch.zeros(E, dtype=torch.uint8, device=dev)
        for _ in range(30):
            env.greedy_actions(out=acts)
            env.step(acts, auto_reset=False, action_format="codes")
        mask = torch.zeros((E, A, 15), dtype=torch.uint8, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        res = (torch.zeros(E, dtype=torch.float64, device=dev), torch.zeros(E, **i32), torch.zeros(E, **i32))

        def greedy_zero():
            env.greedy_init()
            for _ in range(G):
                env.greedy_actions_masked(zeros, out=acts)

        graphs = {"avail_null_us": _graph_of(many(lambda: env.avail_actions(out=mask))),
                  "avail_all_ones_us": _graph_of(many(lambda: env.avail_actions(ones, out=mask))),
                  "avail_all_zero_us": _graph_of(many(lambda: env.avail_actions(zeros, out=mask))),
                  "episode_results_us": _graph_of(many(lambda: env.episode_results(out=res))),
                  "greedy_masked_all_zero_us": _graph_of(greedy_zero)}
        t = {k: [] for k in graphs}
        for _ in range(5):
            for k, g in graphs.items():
                t[k].append(_replay_us(g, reps, G))
        env.avail_actions(out=mask)
        print(json.dumps({"config": "avail_actions", "envs": E, "agents": A, "packages": P, "graph_calls": G,
                          "replays": reps, **t, "mask_bytes": E * A * 15,
                          "masked_fraction": float((mask == 0).float().mean()),
                          "note": "us per call; the greedy graph is [greedy_init, G calls], so its figure carries "
                                  "1/G of one greedy_init"}), flush=True)
        del graphs
        env.close()

    class Agent(torch.nn.Module):
        def __init__(self, dv, hd=64):
            super().__init__()
            self.hd = hd
            self.fc, self.rnn, self.out = torch.nn.Linear(dv, hd), torch.nn.GRUCell(hd, hd), torch.nn.Linear(hd, 15)

        def init_hidden(self):
            return self.fc.weight.new_zeros(1, self.hd)

        def forward(self, so, vo, h):
            h = self.rnn(torch.relu(self.fc(vo)), h)
            return self.out(h), h

    for E in (100, 4096):
        A, P, T, L = 5, 20, 500, 50
        modes = {"off": {}} if collect == "off" else {"off": {}, "on": {"avail": True}}
        cols, envs = {}, []
        torch.manual_seed(0)
        agent = None
        for name, kw in modes.items():
            env = marl_gpu.BatchedEnv(g1, E, A, P, T, seed=42, tracker="fresh", shaping="qmix")
            envs.append(env)
            if agent is None:
                agent = Agent(env.actor_vec_dim).to(dev)
            cols[name] = Q.QmixCollector(env, L, seed=1, **kw)
            cols[name].collect(agent, 0.2, graph=True)      # eager run + capture
            cols[name].collect(agent, 0.2, graph=True)
        n = max(2, steps // 10)
        t = {name: [] for name in cols}
        for _ in range(5):
            for name, col in cols.items():
                t[name].append(timed(lambda k: col.collect(agent, 0.2, graph=True), n) / L)
        print(json.dumps({"config": "avail_qmix_collect", "envs": E, "agents": A, "packages": P, "episode_limit": L,
                          "collects": n, **{f"collect_step_avail_{k}_us": v for k, v in t.items()},
                          "note": "us per env-step of collect(graph=True): reset, observations, L x (agent forward, "
                                  "selection, step_episode), and with avail on L + 1 avail_actions launches"}),
              flush=True)
        for env in envs:
            env.close()


def run_config1(seconds=5.0):
    """BASELINE.json configs[0]: map1, 5 agents, ONE env, a random agent driving the dict
    API (randomagent.py: np.random.choice over moves and ops per robot) -- plumbing, not a
    throughput path.  Here the env is marl_gpu.compat.Environment (every step a kernel
    launch plus the dict snapshot back to the host); reference on CPU: 62,184 agent-steps/s
    with the agent's time, 243,360 env time only (measured in the build
    container).  Settings of SURVEY.md 8(d) row 1: np.random.seed(2025), env seed 2025,
    P = 50, T = 500, reset on done."""
    from marl_gpu.compat import Environment
    env = Environment("map1.txt", max_time_steps=500, n_robots=5, n_packages=50, seed=2025)
    env.reset()
    np.random.seed(2025)
    moves, ops = ["U", "D", "L", "R", "S"], ["0", "1", "2"]
    n, t_env, t0 = 0, 0.0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        acts = [(np.random.choice(moves), np.random.choice(ops)) for _ in range(5)]
        t1 = time.perf_counter()
        _, _, done, _ = env.step(acts)
        if done:
            env.reset()
        t_env += time.perf_counter() - t1
        n += 1
    wall = time.perf_counter() - t0
    print(json.dumps({"config": "1", "envs": 1, "agents": 5, "steps": n,
                      "agent_steps_per_s_with_agent": 5 * n / wall, "agent_steps_per_s_env_only": 5 * n / t_env,
                      "us_per_step_env": t_env / n * 1e6,
                      "note": "compat.Environment (GPU engine, one env) + the reference random agent's action "
                              "draws; reference on CPU: 62,184 / 243,360 agent-steps/s (BASELINE.md)"}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="3,3b,4,5")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--qmix", action="store_true", help="the QMIX episode-collection measurements only")
    ap.add_argument("--idq", action="store_true", help="the IDQ transition-collection measurements only")
    ap.add_argument("--qmix-cycle", action="store_true", help="the map-QMIX cycle-collection measurements only")
    ap.add_argument("--eval", action="store_true", help="the device-resident evaluation measurements only")
    ap.add_argument("--avail", action="store_true", help="the valid-action mask measurements only")
    ap.add_argument("--avail-collect", default="both", choices=["both", "off"],
                    help="with --avail: off = the QMIX collect without the option alone")
    ap.add_argument("--obs-dtype", default="float32",
                    help="float32, float16 or bfloat16 (or several, comma-separated): with a half type, configs 3 / 3b "
                         "print the float32-against-half comparison of one process instead of their usual line, and "
                         "rollout / rollout_graph collect into buffers of that type")
    ap.add_argument("--ego-radius", default="",
                    help="a radius in 1..15 (or several, comma-separated): configs 3 / 5 print the window builder's "
                         "times (build_obs_ego, float32 and bfloat16) beside the full actor maps' instead of their "
                         "usual line")
    ap.add_argument("--ego-active", default="",
                    help="with --ego-radius: a share of the envs in (0, 1] (or several, comma-separated); also time "
                         "build_obs_ego_masked under a fixed mask with that share set")
    ap.add_argument("--ego-collect", type=int, default=0,
                    help="with --ego-radius and --config 5: time QmixCollector(ego_radius=R).collect(graph=True) at "
                         "this many envs instead of the builder (one radius, no --ego-active)")
    ap.add_argument("--alt-ego-radius", default="",
                    help="with --config 5: a window radius 1..15 (or several, comma-separated); time "
                         "build_obs_alt_ego (all envs, and under masks of 1/2 and 1/8 of them) beside build_obs_ego "
                         "in float32 and the full idq_obs build")
    ap.add_argument("--canvas", type=int, nargs=2, metavar=("HC", "WC"), default=None,
                    help="with --config 3 / 5: time build_obs_canvas of the critic map at the map's own shape and at "
                         "HC x WC beside build_obs's critic_map; with --config 4: a graphed mixed-map "
                         "MappoRollout(ego_radius=5, canvas=) beside the single-shape ego rollout (4,096 envs)")
    a = ap.parse_args()
    alt_radii = [int(x) for x in a.alt_ego_radius.split(",") if x]
    if any(not 1 <= r <= 15 for r in alt_radii) or (alt_radii and a.config != "5"):
        ap.error(f"--alt-ego-radius: {a.alt_ego_radius!r} (1..15, with --config 5)")
    radii = [int(x) for x in a.ego_radius.split(",") if x]
    if any(not 1 <= r <= 15 for r in radii):
        ap.error(f"--ego-radius: {a.ego_radius!r} (1..15)")
    active = [float(x) for x in a.ego_active.split(",") if x]
    if any(not 0.0 < f <= 1.0 for f in active) or (active and not radii):
        ap.error(f"--ego-active: {a.ego_active!r} (shares in (0, 1], with --ego-radius)")
    obs_dtypes = a.obs_dtype.split(",")
    if any(n not in OBS_DTYPES for n in obs_dtypes):
        ap.error(f"--obs-dtype: {a.obs_dtype!r} (float32, float16, bfloat16)")
    half = [n for n in obs_dtypes if n != "float32"]
    torch.cuda.set_device(0)
    if a.avail:
        run_avail(a.steps, a.avail_collect)
        return
    if a.eval:
        run_eval_bench(a.steps)
        return
    if a.qmix:
        run_qmix(a.steps)
        return
    if a.idq:
        run_idq(a.steps)
        return
    if a.qmix_cycle:
        run_qmix_cycle(a.steps)
        return
    if alt_radii:
        run_alt_ego(alt_radii, a.steps, a.warmup)
        return
    for c in a.config.split(","):
        if c == "1":
            run_config1()
        elif c in ("rollout", "rollout_graph"):
            for n in obs_dtypes:
                run_rollout(a.steps, graph=c == "rollout_graph", obs_dtype=n)
        elif c == "alt":
            run_alt(a.steps)
        elif c == "greedy":
            run_greedy(a.steps)
        elif a.canvas:
            run_canvas(c, tuple(a.canvas), a.steps, a.warmup)
        elif radii and a.ego_collect:
            if c != "5" or len(radii) != 1 or active:
                ap.error("--ego-collect goes with --config 5 and one --ego-radius, without --ego-active")
            run_ego_collect(a.ego_collect, radii[0], a.steps)
        elif radii:
            run_ego(c, radii, a.steps, a.warmup, active=active)
        elif c in ("3", "3b") and half:
            run_obs_dtype(c, a.steps, a.warmup, half)
        else:
            run(c, a.steps, a.warmup)


if __name__ == "__main__":
    main()
