"""The batched view entry points of the C ABI (mdl_views_features, mdl_views_shaped_reward,
mdl_views_alt_features, mdl_views_idq_reward and the two mdl_host_views_* forms) on many distinct records
per launch, against the oracle, bit for bit: per-view offsets into irregularly packed blobs, views with fewer
slots than max_slots (down to none), views on every map of a multi-map engine, mixed robot counts, agent
indices out of range, launches of one view, of a partial workgroup and of several workgroups.  Every output
carries two guard rows past the last view, which must come back untouched.  The inputs and the expected
values are tests/views_ref.py's; tests/test_views_batch_cpu.py holds the conditions they satisfy."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import oracle as O  # noqa: E402
import views_ref as V  # noqa: E402

SENT32 = 0x7FC0BEEF              # a NaN payload no builder writes
SENT64 = 0x7FF8DEADBEEF0001
GUARD = 2                        # rows past the last view
FEATURES = ("obs", "vec", "gmap", "gvec")


@pytest.fixture(scope="module")
def dev():
    """The multi-map engine (it only supplies the maps) and the three blobs on the device."""
    import marl_gpu
    p = V.pool()
    env = marl_gpu.BatchedEnv(list(V.maps()), len(V.maps()), env_map=list(range(len(V.maps()))), shaping="qmix")
    d = dict(env=env, prev=torch.from_numpy(p.prev).cuda(), cur=torch.from_numpy(p.cur).cuda(),
             act=torch.from_numpy(p.act).cuda())
    yield d
    env.close()


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(n, row, wide=False):
    """(n + GUARD) rows of `row` sentinel words on the device."""
    return torch.full(((n + GUARD) * row,), SENT64 if wide else SENT32, dtype=torch.int64 if wide else torch.int32,
                      device="cuda")


def _take(t, n, row, dtype=np.float32):
    """The n rows of a guarded output, after checking that the guard rows were not written."""
    a = t.cpu().numpy()
    assert (a[n * row:] == (SENT32 if a.dtype == np.int32 else SENT64)).all(), "a write past the last view's row"
    return a[:n * row].view(dtype).reshape(n, row)


def _same(got, want, what):
    want = np.ascontiguousarray(want).reshape(got.shape)
    np.testing.assert_array_equal(got, want, err_msg=str(what))
    assert got.tobytes() == want.tobytes(), what


def _feature_rows(shape, sizes):
    (H, W), (MO, MP, MR, MPs) = shape, sizes
    return dict(obs=6 * H * W, vec=6 + 5 * MO + 5 * MP + 1, gmap=4 * H * W, gvec=6 * MR + 7 * MPs + 1)


def _run_features(d, b, sizes, want=FEATURES, order=None):
    from marl_gpu._lib import check, lib, ptr, stream_handle
    p = V.pool()
    order = np.arange(b.n) if order is None else order
    offs, agent = _cuda(p.prev_off[b.idx[order]]), _cuda(b.agent[order])
    rows = _feature_rows(b.shape, sizes)
    out = {k: _guarded(b.n, rows[k]) for k in want}
    check(lib().mdl_views_features(d["env"]._h, ptr(d["prev"]), ptr(offs), b.n, b.max_slots, ptr(agent), V.T, *sizes,
                                   *[ptr(out.get(k)) for k in FEATURES], stream_handle()), "mdl_views_features")
    torch.cuda.synchronize()
    return {k: _take(out[k], b.n, rows[k]) for k in want}


@pytest.mark.parametrize("name", V.FEATURE_BATCHES)
def test_views_features(dev, name):
    b = V.batches()[name]
    for sizes in b.sizes():
        exp = V.features(name, sizes)
        for want in (FEATURES, ("vec",), ("obs",)):
            got = _run_features(dev, b, sizes, want)
            for k in want:
                _same(got[k], exp[k], (name, sizes, want, k))


def test_views_features_reversed(dev):
    """The same views in reversed order (offsets and agent indices reversed, the blob as it was): row
    n-1-w is the earlier row w."""
    b = V.batches()["large-37"]
    sizes = b.sizes()[2]
    first = _run_features(dev, b, sizes)
    again = _run_features(dev, b, sizes, order=np.arange(b.n)[::-1])
    for k in FEATURES:
        _same(again[k][::-1], first[k], k)
        _same(first[k], V.features("large-37", sizes)[k], k)


def _run_shaped(d, b, consts):
    from marl_gpu._lib import check, lib, ptr, stream_handle
    p = V.pool()
    po, co, ao, g = (_cuda(x[b.idx]) for x in (p.prev_off, p.cur_off, p.act_off, p.g))
    out = _guarded(b.n, 1)
    cs = None if consts is None else (C.c_double * 9)(*V.CONSTS[consts])
    check(lib().mdl_views_shaped_reward(d["env"]._h, ptr(d["prev"]), ptr(po), b.max_slots, ptr(d["cur"]), ptr(co),
                                        ptr(d["act"]), ptr(ao), ptr(g), b.n, None if cs is None else C.addressof(cs),
                                        ptr(out), stream_handle()), "mdl_views_shaped_reward")
    torch.cuda.synchronize()
    return _take(out, b.n, 1)[:, 0]


@pytest.mark.parametrize("name", V.REWARD_BATCHES)
def test_views_shaped_reward(dev, name):
    """Views of both map shapes in one launch; the constants as an array, and the engine's own (qmix)."""
    b = V.batches()[name]
    for consts, exp in (("mappo", "mappo"), ("qmix", "qmix"), (None, "qmix")):
        _same(_run_shaped(dev, b, consts), V.shaped(name, exp), (name, consts))


def _run_alt(d, b, shape, want, order=None):
    from marl_gpu._lib import check, lib, ptr, stream_handle
    p = V.pool()
    order = np.arange(b.n) if order is None else order
    offs, agent = _cuda(p.prev_off[b.idx[order]]), _cuda(b.agent[order])
    rows = dict(idq=6 * b.shape[0] * b.shape[1], qmix=7 * shape[1] * shape[2])
    out = {k: _guarded(b.n, rows[k]) for k in want}
    check(lib().mdl_views_alt_features(d["env"]._h, ptr(d["prev"]), ptr(offs), b.n, b.max_slots, ptr(agent),
                                       ptr(out.get("idq")), ptr(out.get("qmix")), shape[1], shape[2], stream_handle()),
          "mdl_views_alt_features")
    torch.cuda.synchronize()
    return {k: _take(out[k], b.n, rows[k]) for k in want}


@pytest.mark.parametrize("name", V.FEATURE_BATCHES)
def test_views_alt_features(dev, name):
    b = V.batches()[name]
    for shape in V.alt_shapes(name):
        exp = V.alt(name, shape)
        for want in (("idq", "qmix"), ("idq",), ("qmix",)):
            got = _run_alt(dev, b, shape, want)
            for k in want:
                _same(got[k], exp[k], (name, shape, want, k))
    if b.n == 37:
        shape = V.alt_shapes(name)[1]
        got = _run_alt(dev, b, shape, ("idq", "qmix"), order=np.arange(b.n)[::-1])
        for k in ("idq", "qmix"):
            _same(got[k][::-1], V.alt(name, shape)[k], (name, "reversed", k))


@pytest.mark.parametrize("name", V.REWARD_BATCHES)
def test_views_idq_reward(dev, name):
    """out[op_offsets[w] + a] per agent, with the views' entries spaced further apart than their robot
    counts: the entries between them, before the first and past the last stay untouched.  The guard past
    the last entry is n * max(A) long: every entry a view-number stride could reach lies inside it."""
    from marl_gpu._lib import check, lib, ptr, stream_handle
    p = V.pool()
    b = V.batches()[name]
    po, co, oo, ops = _cuda(p.prev_off[b.idx]), _cuda(p.cur_off[b.idx]), _cuda(b.op_off), _cuda(b.ops())
    for ints in (True, False):
        total = b.op_total + b.n * int(b.A.max())
        out = _guarded(total - GUARD, 1, wide=True)
        check(lib().mdl_views_idq_reward(dev["env"]._h, ptr(dev["prev"]), ptr(po), b.max_slots, ptr(dev["cur"]),
                                         ptr(co), ptr(ops), ptr(oo), int(ints), b.n, ptr(out), stream_handle()),
              "mdl_views_idq_reward")
        torch.cuda.synchronize()
        got = _take(out, total - GUARD, 1, np.float64)[:, 0]
        want, written = np.zeros(got.size), np.zeros(got.size, bool)
        for w, r in enumerate(V.idq_reward(name, ints)):
            want[b.op_off[w]:b.op_off[w] + b.A[w]] = r
            written[b.op_off[w]:b.op_off[w] + b.A[w]] = True
        assert (got.view(np.int64)[~written] == SENT64).all(), (name, ints, "a write outside the views' entries")
        _same(got[written], want[written], (name, ints))


# ------------------------------------------------------------------ the host forms
def _align(x, a=16):
    return (x + a - 1) // a * a


class _Arena:
    """Sections laid out one after another in the helper engine's host-mapped arena."""

    def __init__(self, grid):
        from marl_gpu import helper
        self.ar = helper._arena_for(grid)
        self.parts, self.pos = [], 0

    def add(self, a=None, nbytes=None):
        """Reserve a section (16-byte aligned) holding array `a`, or `nbytes` of sentinel words."""
        nbytes = a.nbytes if a is not None else nbytes
        self.parts.append((self.pos, a, nbytes))
        self.pos = _align(self.pos + nbytes)
        return len(self.parts) - 1

    def fill(self):
        u8 = self.ar.get(self.pos)
        for off, a, nbytes in self.parts:
            if a is not None:
                u8[off:off + nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
            else:
                u8[off:off + nbytes].view(np.int32)[:] = SENT32
        self.u8 = u8

    def addr(self, k):
        return self.ar.addr + self.parts[k][0]

    def words(self, k):
        off, _, nbytes = self.parts[k]
        return self.u8[off:off + nbytes].view(np.int32).copy()


def _packed(b):
    """The batch's own records back to back (prev, cur, action bytes) with their offsets."""
    p = V.pool()
    prev, cur, act = [], [], []
    for i in b.idx:
        prev.append(p.prev[p.prev_off[i]:p.prev_off[i] + 4 + 3 * p.A[i] + 8 * p.ns[i]])
        cur.append(p.cur[p.cur_off[i]:p.cur_off[i] + 2 + 3 * p.A[i]])
        act.append(p.act[p.act_off[i]:p.act_off[i] + p.A[i]])

    def offs(parts):
        return (np.cumsum([x.size for x in parts]) - [x.size for x in parts]).astype(np.int64)
    return (np.concatenate(prev), offs(prev)), (np.concatenate(cur), offs(cur)), (np.concatenate(act), offs(act))


@pytest.mark.parametrize("name", ["small-5", "small-37"])
def test_host_views(name):
    """mdl_host_views_features / _shaped_reward on n distinct records in the helper engine's arena (its
    single map: the batches of map 0), then a single-view helper call on the same engine: the completion
    counting of a launch of several waves leaves the next call's completion word right."""
    from marl_gpu import helper
    from marl_gpu._lib import check, lib
    b = V.batches()[name]
    grid = V.maps()[0]
    assert (b.map == 0).all()
    (prev, po), (cur, co), (act, ao) = _packed(b)
    for sizes in b.sizes():
        rows = _feature_rows(b.shape, sizes)
        A = _Arena(grid)
        k_prev, k_off, k_idx = A.add(prev), A.add(po), A.add(b.agent)
        k_out = {k: A.add(nbytes=4 * (b.n + GUARD) * rows[k]) for k in FEATURES}
        A.fill()
        check(lib().mdl_host_views_features(A.ar.eng._h, A.addr(k_prev), A.addr(k_off), b.n, b.max_slots, A.addr(k_idx),
                                            V.T, *sizes, *[A.addr(k_out[k]) for k in FEATURES], A.ar.stream),
              "mdl_host_views_features")
        exp = V.features(name, sizes)
        for k in FEATURES:
            w = A.words(k_out[k])
            assert (w[b.n * rows[k]:] == SENT32).all(), (name, sizes, k, "a write past the last view's row")
            _same(w[:b.n * rows[k]].view(np.float32).reshape(b.n, rows[k]), exp[k], (name, sizes, k))
    for consts in ("mappo", "qmix"):
        A = _Arena(grid)
        ks = [A.add(x) for x in (prev, po, cur, co, act, ao, V.pool().g[b.idx])]
        k_out = A.add(nbytes=4 * (b.n + GUARD))
        A.fill()
        cs = (C.c_double * 9)(*V.CONSTS[consts])
        check(lib().mdl_host_views_shaped_reward(A.ar.eng._h, A.addr(ks[0]), A.addr(ks[1]), b.max_slots, A.addr(ks[2]),
                                                 A.addr(ks[3]), A.addr(ks[4]), A.addr(ks[5]), A.addr(ks[6]), b.n,
                                                 C.addressof(cs), A.addr(k_out), A.ar.stream),
              "mdl_host_views_shaped_reward")
        w = A.words(k_out)
        assert (w[b.n:] == SENT32).all()
        _same(w[:b.n].view(np.float32), V.shaped(name, consts), (name, consts))
    x = V.pool().trans[b.idx[0]]
    r1 = x["rob0"].copy()
    r1[:, :2] += 1
    state = {"time_step": x["t0"], "map": grid, "robots": [tuple(int(v) for v in r) for r in r1], "packages": []}
    for a in range(x["A"]):
        _same(helper.convert_observation(state, x["rows0"].tolist(), a),
              O.convert_observation(grid, x["t0"], r1, x["rows0"], a), (name, "convert_observation after", a))
