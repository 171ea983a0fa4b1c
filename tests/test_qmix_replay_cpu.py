"""``EpisodeReplay`` (the QMIX episode ring, QMIX/networks.py:209-318) on CPU tensors with a
hand-made batch: ring wrap and eviction, the reference's sample dictionary, the shifted
``*_next`` views and the padding mask.  No GPU: the ring is plain torch ops."""
import pytest

torch = pytest.importorskip("torch")

L, E, A, H, W, DV, DG, NA = 5, 4, 3, 2, 3, 7, 9, 15


def _replay_cls():
    from marl_gpu.qmix_rollout import EpisodeReplay
    return EpisodeReplay


def make_batch(tag):
    """E episodes whose every value names (tag, env, slot): so[t, e] == 1000 tag + 10 e + t."""
    def obs(*tail):
        t = torch.arange(L + 1, dtype=torch.float32).reshape(L + 1, 1, *[1] * len(tail))
        e = torch.arange(E, dtype=torch.float32).reshape(1, E, *[1] * len(tail))
        return (1000.0 * tag + 10.0 * e + t).expand(L + 1, E, *tail).contiguous()

    lengths = torch.tensor([L, 2, 1, 4])
    steps = torch.arange(L).reshape(L, 1)
    filled = (steps < lengths.reshape(1, E)).to(torch.uint8)
    terminated = ((steps == lengths.reshape(1, E) - 1) & (lengths.reshape(1, E) < L)).to(torch.uint8)
    return dict(so=obs(A, 6, H, W), vo=obs(A, DV), gs=obs(4, H, W), gv=obs(DG),
                u=((steps.reshape(L, 1, 1) + torch.arange(E).reshape(1, E, 1) + tag) % NA).expand(L, E, A)
                .to(torch.uint8).contiguous(),
                r=(100.0 * tag + obs()[:L]).contiguous(), terminated=terminated, filled=filled)


def test_ring_wraps_and_evicts_oldest():
    R = _replay_cls()(10, make_batch(0), n_actions=NA)
    assert len(R) == 0
    for tag in range(3):   # 12 episodes into 10 slots
        R.add(make_batch(tag))
    assert len(R) == 10 and R.idx == 2
    tags = (R.buf["so"][0, :, 0, 0, 0, 0] // 1000).tolist()
    envs = ((R.buf["so"][0, :, 0, 0, 0, 0] % 1000) // 10).tolist()
    # slots 0, 1: the last two episodes of batch 2 (they evicted batch 0's envs 0, 1); then batch 0's
    # envs 2, 3, batch 1, and batch 2's envs 0, 1 -- env order inside every batch
    assert tags == [2, 2, 0, 0, 1, 1, 1, 1, 2, 2]
    assert envs == [2, 3, 2, 3, 0, 1, 2, 3, 0, 1]


def test_sample_matches_reference_dictionary():
    R = _replay_cls()(8, make_batch(0), n_actions=NA)
    with pytest.raises(ValueError):
        R.sample(1)                      # nothing stored yet
    R.add(make_batch(1))
    with pytest.raises(ValueError):
        R.sample(5)                      # 4 episodes stored
    R.add(make_batch(2))
    B = 6
    s = R.sample(B, generator=torch.Generator().manual_seed(0))
    want = {"so": (B, L, A, 6, H, W), "vo": (B, L, A, DV), "gs": (B, L, 4, H, W), "gv": (B, L, DG),
            "u": (B, L, A, 1), "r": (B, L, 1), "so_next": (B, L, A, 6, H, W), "vo_next": (B, L, A, DV),
            "gs_next": (B, L, 4, H, W), "gv_next": (B, L, DG), "avail_u": (B, L, A, NA),
            "avail_u_next": (B, L, A, NA), "terminated": (B, L, 1), "padded": (B, L, 1)}
    assert set(s) == set(want)           # QMIX/networks.py:299-314
    for k, shape in want.items():
        assert tuple(s[k].shape) == shape, k
        assert s[k].dtype == (torch.int64 if k == "u" else torch.float32), k
    assert (s["avail_u"] == 1).all() and (s["avail_u_next"] == 1).all()
    # distinct episodes: (tag, env) identifies one
    ident = s["so"][:, 0, 0, 0, 0, 0].tolist()
    assert len(set(ident)) == B
    # *_next is the slots shifted by one
    for k in ("so", "vo", "gs", "gv"):
        assert torch.equal(s[k + "_next"][:, :-1], s[k][:, 1:]), k
        assert torch.equal(s[k + "_next"][:, -1] - s[k][:, -1], torch.ones_like(s[k][:, -1])), k
        assert s[k + "_next"].data_ptr() != s[k].data_ptr()
        assert s[k + "_next"].untyped_storage().data_ptr() == s[k].untyped_storage().data_ptr(), "one gathered copy"
    # every sampled episode against its source batch
    for b in range(B):
        tag, e = int(ident[b] // 1000), int((ident[b] % 1000) // 10)
        src = make_batch(tag)
        assert torch.equal(s["so"][b], src["so"][:L, e]) and torch.equal(s["so_next"][b], src["so"][1:, e])
        assert torch.equal(s["gv"][b], src["gv"][:L, e])
        assert torch.equal(s["u"][b, :, :, 0], src["u"][:, e].long())
        assert torch.equal(s["r"][b, :, 0], src["r"][:, e])
        assert torch.equal(s["terminated"][b, :, 0], src["terminated"][:, e].float())
        assert torch.equal(s["padded"][b, :, 0], 1.0 - src["filled"][:, e].float())


def test_sample_is_without_replacement_and_seeded():
    R = _replay_cls()(4, make_batch(0), n_actions=NA)
    R.add(make_batch(3))
    a = R.sample(4, generator=torch.Generator().manual_seed(5))
    b = R.sample(4, generator=torch.Generator().manual_seed(5))
    assert torch.equal(a["so"], b["so"])
    assert sorted(((a["so"][:, 0, 0, 0, 0, 0] % 1000) // 10).tolist()) == [0, 1, 2, 3]
