"""GPU (-m gpu): the training step fed by SENSOR frames (pnvo_train_forward_raw, pnvo_input_moments_raw, pnvo_dataset_frames and
the Python methods above them) against the materialised path it replaces — pnvo_build_obs_pairs followed by the pair entry
points.  The same values reach the stem forward and its weight gradient (uint8 rgb is exact, the one-hot depth is derived with
the reference's own comparisons and the caller's edges), so outputs and gradients must be IDENTICAL bit for bit; the moments
are held to two float32 ulps of a float64 sum of the same float32 terms; the whole step is held to tests/test_gpu_train.py's own
bounds against the fp64 checker."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import golden_case, load_golden
from oracle import torch_train_ref as ref
from pointnav_vo_amd import _lib, model_spec as ms, synth, vo_cnn  # noqa: F401
from pointnav_vo_amd.dataset import StatePairBatcher
from pointnav_vo_amd.registry import baseline_registry
from pointnav_vo_amd.train import GeoInvarianceTrainStep, VOTrainStep
from pointnav_vo_amd.trainer import NormalizedDepth2TopDownViewHabitatTorch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPACE = ["rgb", "depth", "discretized_depth", "top_down_view"]
GRAD_TOL = 3e-5                                   # tests/test_gpu_train.py
E32 = np.array([np.float32(i / 10) for i in range(10)] + [1.0], dtype=np.float32)              # the navigation boundary's edges
E16 = np.array([np.float32(np.float16(i / 10)) for i in range(10)] + [1.0], dtype=np.float32)  # the dataset's (StatePairBatcher.edges)


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def build_model(name, space, W, H, seed, bins=10):
    kw = dict(observation_space=space, observation_size=(W, H), hidden_size=512, backbone="resnet18", normalize_visual_inputs=True,
              output_dim=3, dropout_p=0.0)
    if bins:
        kw["discretized_depth_channels"] = bins
    m = baseline_registry.get_vo_model(name)(**kw)
    sd = synth.make_state_dict(ms.state_dict_spec(m.cfg), seed=seed)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    return m.to(DEV)


def plant_edges(dep):
    """Every edge of both edge sets, one float32 above and below each, and the closed ends 0 and 1 (W >= 31)."""
    row = 5
    for e in (E32, E16):
        vals = np.concatenate([e, np.nextafter(e, np.float32(2))[:-1], np.nextafter(e, np.float32(-1))[1:]])
        dep[0, 0, row, : vals.size] = vals
        dep[0, 1, row + 2, : vals.size] = vals[::-1]
        dep[-1, 1, -1 - row, -vals.size:] = vals                      # ... and in the last rows of the last frame
        row += 4


def frames(n, H, W, seed, depth_edit=plant_edges):
    """device tensors: rgb uint8 [n,2,H,W,3], depth float32 [n,2,H,W] (pair i = frames i, i + 1 of a synthetic walk)."""
    obs = [synth.make_raw_obs(H, W, seed=seed, index=i, zero_border=3 * (i % 3 == 0)) for i in range(n + 1)]
    rgb = np.stack([np.stack([obs[i]["rgb"], obs[i + 1]["rgb"]]) for i in range(n)])
    dep = np.stack([np.stack([obs[i]["depth"][..., 0], obs[i + 1]["depth"][..., 0]]) for i in range(n)]).astype(np.float32)
    if depth_edit is not None:
        depth_edit(dep)
    return torch.from_numpy(rgb).to(DEV), torch.from_numpy(dep).to(DEV)


def onehot(dep, edges):
    """[n,2,H,W] depth frames -> [n,H,W,20] one-hot pair tensor: e_i <= d < e_{i+1}, last bin closed (float32 comparisons)."""
    e = torch.as_tensor(np.asarray(edges, dtype=np.float32), device=dep.device)
    d = dep.permute(0, 2, 3, 1).unsqueeze(-1)                          # [n,H,W,2,1]
    hit = (d >= e[:-1]) & (d < e[1:])
    hit[..., -1] = (d[..., 0] >= e[-2]) & (d[..., 0] <= e[-1])
    return hit.to(torch.float32).reshape(*hit.shape[:3], 2 * (e.numel() - 1)).contiguous()


def materialise(rgb, dep, H, W, bins, want_tdv=True, edges=None):
    """pnvo_build_obs_pairs: the observation-pair tensors of the reference boundary, on the device (the one-hot depth rebuilt with
    `edges` when they are not the boundary's)."""
    n = dep.shape[0]
    gen = NormalizedDepth2TopDownViewHabitatTorch(min_depth=0.1, max_depth=10.0, vis_size_h=H, vis_size_w=W, hfov_rad=70)
    o = {"rgb": torch.empty((n, H, W, 6), device=DEV) if rgb is not None else None, "depth": torch.empty((n, H, W, 2), device=DEV),
         "discretized_depth": torch.empty((n, H, W, 2 * bins), device=DEV) if bins else None,
         "top_down_view": torch.empty((n, H, W, 2), device=DEV) if want_tdv else None}
    work = torch.empty(int(_lib.lib.pnvo_topdown_workspace_bytes(n, H, W)), dtype=torch.uint8, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib.pnvo_build_obs_pairs(p(rgb), p(dep), n, H, W, bins, gen._consts, int(gen._rows_around_center), p(work), p(o["rgb"]),
                                             p(o["depth"]), p(o["discretized_depth"]), p(o["top_down_view"]), p(flag), stream()))
    if bins and edges is not None:
        o["discretized_depth"] = onehot(dep, edges)
    assert int(flag) == 0
    return {k: v for k, v in o.items() if v is not None}


def c_edges(edges):
    return None if edges is None else (C.c_float * len(edges))(*[float(x) for x in edges])


def pair_and_frame_passes(model, space, obs, rgb, dep, tdv, edges):
    """On ONE handle, with the SAME run_mean / run_var tensors: pnvo_train_forward + pnvo_train_backward on the pair tensors, then
    pnvo_train_forward_raw + pnvo_train_backward on the frames.  -> ((out, grad) of the pairs, (out, grad) of the frames)."""
    ts = VOTrainStep(model)
    h = model._handle
    B = dep.shape[0]
    rmv = model.visual_encoder.running_mean_and_var
    mean, var = rmv._mean.reshape(-1).float().contiguous(), rmv._var.reshape(-1).float().contiguous()
    gout = torch.from_numpy(synth.uniform(3, "gout", (B, 3), -1.0, 1.0).astype(np.float32)).to(DEV)
    ptrs = [p(obs[k]) if k in space else None for k in ("rgb", "depth", "discretized_depth", "top_down_view")]
    res = []
    for form in ("pairs", "frames"):
        out = torch.full((B, 3), float("nan"), device=DEV)
        ts.grad.fill_(float("nan"))                                     # (the backward overwrites the whole buffer)
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        if form == "pairs":
            _lib.check(_lib.lib.pnvo_train_forward(h, *ptrs, B, p(mean), p(var), p(out), stream()), h)
        else:
            _lib.check(_lib.lib.pnvo_train_forward_raw(h, p(rgb) if "rgb" in space else None, p(dep), p(tdv), c_edges(edges), B, p(mean),
                                                       p(var), p(out), p(err), stream()), h)
        _lib.check(_lib.lib.pnvo_train_backward(h, p(gout), stream()), h)
        torch.cuda.synchronize()
        assert int(err) == 0
        res.append((out.clone(), ts.grad.clone()))
    return res


def assert_identical(a, b):
    assert torch.isfinite(a[0]).all() and torch.isfinite(a[1]).all()
    assert torch.equal(a[0], b[0]), (a[0] - b[0]).abs().max()
    assert torch.equal(a[1], b[1]), (int((a[1] != b[1]).sum()), (a[1] - b[1]).abs().max())


@pytest.mark.parametrize("edges", [None, E16], ids=["edges_f32", "edges_f16"])
@pytest.mark.parametrize("W,H,B", [(98, 66, 3), (341, 192, 2)])
def test_train_forward_raw_and_backward_equal_the_pair_path_bit_for_bit(W, H, B, edges):
    """The default 30-channel model.  98x66: the stem map is 33x49, partial tiles on both axes of the 6x13 wgrad tile, and a frame is
    19 404 B, so every frame starts at another alignment; 341x192: the real row stride.  Depth carries every edge +-1 ulp."""
    model = build_model("vo_cnn_rgb_d_dd_top_down", SPACE, W, H, seed=4)
    rgb, dep = frames(B, H, W, seed=11)
    obs = materialise(rgb, dep, H, W, 10, edges=edges)
    pairs, frm = pair_and_frame_passes(model, SPACE, obs, rgb, dep, obs["top_down_view"], edges)
    assert_identical(pairs, frm)
    if edges is not None:                             # the edges matter: some planted depth changes its bin between the two sets
        assert not torch.equal(obs["discretized_depth"], onehot(dep, E32))


def test_train_forward_raw_on_three_bf16_pieces():
    """Option train_pieces=3: the training forward's stem runs its three-piece form from the frames."""
    H, W, B = 66, 98, 3
    model = build_model("vo_cnn_rgb_d_dd_top_down", SPACE, W, H, seed=4)
    model.set_option("train_pieces", "3")
    rgb, dep = frames(B, H, W, seed=11)
    obs = materialise(rgb, dep, H, W, 10)
    pairs, frm = pair_and_frame_passes(model, SPACE, obs, rgb, dep, obs["top_down_view"], None)
    assert_identical(pairs, frm)


@pytest.mark.parametrize("name,space,bins", [("vo_cnn", ["rgb", "depth"], 0),
                                             ("vo_cnn_d_dd_top_down", ["depth", "discretized_depth", "top_down_view"], 10),
                                             ("vo_cnn_rgb_d_dd", ["rgb", "depth", "discretized_depth"], 10),
                                             ("vo_cnn_rgb_d_top_down", ["rgb", "depth", "top_down_view"], 0),
                                             ("vo_cnn_rgb_dd_top_down", ["rgb", "discretized_depth", "top_down_view"], 10)])
def test_train_forward_raw_on_models_with_fewer_modalities(name, space, bins):
    """No one-hot and no top-down view; no rgb frames; no top-down view; no one-hot; the one-hot without the depth tensor (the depth
    frames are still what it is derived from).  The pair path compared against is held to fp64 on each of these layouts by
    tests/test_gpu_train_models.py."""
    H, W, B = 66, 98, 3
    model = build_model(name, space, W, H, seed=6, bins=bins)
    rgb, dep = frames(B, H, W, seed=13)
    obs = materialise(rgb if "rgb" in space else None, dep, H, W, bins, want_tdv="top_down_view" in space)
    pairs, frm = pair_and_frame_passes(model, space, obs, rgb, dep, obs.get("top_down_view"), None)
    assert_identical(pairs, frm)


def test_frames_inside_larger_allocations_give_the_same_bits():
    """Guard band: the frame tensors are slices in the middle of larger allocations whose other bytes are 0xFF (rgb) and NaN (depth,
    top-down view) — a piece read outside the tensors would reach the operands."""
    H, W, B = 66, 98, 3
    model = build_model("vo_cnn_rgb_d_dd_top_down", SPACE, W, H, seed=4)
    rgb, dep = frames(B, H, W, seed=11)
    obs = materialise(rgb, dep, H, W, 10)

    def inside(t, pad, fill):
        big = torch.full((t.numel() + 2 * pad,), fill, dtype=t.dtype, device=DEV)
        big[pad:pad + t.numel()] = t.reshape(-1)
        return big[pad:pad + t.numel()].view(t.shape), big

    grgb, k0 = inside(rgb, 37, 255)                   # 37 B: no alignment at all
    gdep, k1 = inside(dep, 5, float("nan"))           # 20 B: 4-byte aligned only
    gtdv, k2 = inside(obs["top_down_view"], 6, float("nan"))
    assert grgb.is_contiguous() and gdep.is_contiguous() and gtdv.is_contiguous()
    pairs, frm = pair_and_frame_passes(model, SPACE, obs, grgb, gdep, gtdv, None)
    assert_identical(pairs, frm)
    assert bool((k0[:37] == 255).all()) and bool(torch.isnan(k1[:5]).all())          # (and nothing wrote there)


def test_input_moments_raw_within_two_ulps_of_the_float64_sum():
    """power 3, non-zero centre: each of the 2C outputs against a float64 numpy sum of the same float32 terms.  The fp64 partial sums
    contribute nothing at this size and the final cast half an ulp; the pair kernel is held to the same bound."""
    H, W, B = 66, 98, 3
    model = build_model("vo_cnn_rgb_d_dd_top_down", SPACE, W, H, seed=4)
    ts = VOTrainStep(model)                          # (attaches the training state the moments' scratch belongs to)
    assert ts.n_params > 0
    h, Cc = model._handle, model.cfg.in_channels
    rgb, dep = frames(B, H, W, seed=11)
    obs = materialise(rgb, dep, H, W, 10, edges=E16)
    center = torch.from_numpy(synth.uniform(5, "centre", (Cc,), 0.05, 0.6).astype(np.float32)).to(DEV)
    got_f, got_p = torch.empty(2 * Cc, device=DEV), torch.empty(2 * Cc, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib.pnvo_input_moments_raw(h, p(rgb), p(dep), p(obs["top_down_view"]), c_edges(E16), B, p(center), 3, p(got_f), p(err),
                                               stream()), h)
    _lib.check(_lib.lib.pnvo_input_moments(h, p(obs["rgb"]), p(obs["depth"]), p(obs["discretized_depth"]), p(obs["top_down_view"]), B,
                                           p(center), 3, p(got_p), stream()), h)
    torch.cuda.synchronize()
    assert int(err) == 0
    # the assembled input in reference channel order [prev rgb, d, one-hot, tdv | cur ...], rgb / 255 in float32
    o = {k: v.cpu().numpy() for k, v in obs.items()}
    half = lambda f: [o["rgb"][..., 3 * f:3 * f + 3] / np.float32(255.0), o["depth"][..., f:f + 1],
                      o["discretized_depth"][..., 10 * f:10 * f + 10], o["top_down_view"][..., f:f + 1]]
    x = np.concatenate(half(0) + half(1), axis=-1)
    assert x.dtype == np.float32 and x.shape[-1] == Cc
    t = (x - center.cpu().numpy()).astype(np.float32).astype(np.float64).reshape(-1, Cc)     # the float32 terms, exactly
    want = np.concatenate([t.mean(0), (t * t).mean(0)])
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    for name, got in (("frames", got_f), ("pairs", got_p)):
        d = np.abs(got.cpu().numpy().astype(np.float64) - want) / ulp
        print(f"moments ({name}): worst {d.max():.3f} ulp")
        assert d.max() <= 2.0, (name, d)


@functools.lru_cache(maxsize=None)
def fixture_case(fname):
    """A training fixture turned into frames, and the fp64 checker's step on it (computed once)."""
    rec = load_golden(fname)
    cfg, sd, obs, _ = golden_case(rec)
    B, H, W = obs["depth"].shape[:3]
    # possible because the fixture holds integer rgb in 0..255 and its one-hot depth is that of its depth under float32(i / 10) edges
    assert np.array_equal(obs["rgb"], obs["rgb"].astype(np.uint8).astype(np.float32))
    rgb = np.ascontiguousarray(obs["rgb"].astype(np.uint8).reshape(B, H, W, 2, 3).transpose(0, 3, 1, 2, 4))
    dep = np.ascontiguousarray(obs["depth"].transpose(0, 3, 1, 2))
    assert np.array_equal(onehot(torch.from_numpy(dep), E32).numpy(), obs["discretized_depth"])
    chk = ref.train_step(sd, obs, rec["target"], ngroups=cfg.ngroups, lr=float(rec["lr"]), eps=float(rec["eps"]), dtype=torch.float64)
    return rec, cfg, sd, obs, rgb, dep, chk


@pytest.mark.parametrize("fname", ["train_default_96x64_b3_f32.npz", "train_default_45x37_b4_f64.npz"])
def test_step_raw_matches_the_fp64_checker(fname):
    rec, cfg, sd, obs, rgb, dep, chk = fixture_case(fname)
    space = str(rec["obs_space"]).split(",")
    model = baseline_registry.get_vo_model(str(rec["model"]))(
        observation_space=space, observation_size=(cfg.width, cfg.height), hidden_size=512, backbone="resnet18",
        normalize_visual_inputs=True, output_dim=3, dropout_p=0.0, discretized_depth_channels=int(rec["dd_bins"]))
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    model = model.to(DEV)
    ts = VOTrainStep(model, lr=float(rec["lr"]), eps=float(rec["eps"]))
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    out, loss = ts.step_raw(torch.from_numpy(rgb).to(DEV), torch.from_numpy(dep).to(DEV), torch.from_numpy(obs["top_down_view"]).to(DEV),
                            target=torch.from_numpy(rec["target"]).to(DEV), err_flag=err)
    torch.cuda.synchronize()
    assert int(err) == 0
    np.testing.assert_allclose(out.cpu().numpy(), rec["out1"], rtol=2e-4, atol=2e-5)
    assert abs(loss.item() - float(rec["loss1"])) < 1e-4 * max(1.0, abs(float(rec["loss1"])))
    for k in ("_mean", "_var", "_count"):
        b = getattr(model.visual_encoder.running_mean_and_var, k).cpu().double().numpy().reshape(-1)
        np.testing.assert_allclose(b, rec[f"buf1/visual_encoder.running_mean_and_var.{k}"].reshape(-1), rtol=1e-5, atol=1e-6)
    bad = []
    for name, (off, n) in ts.offsets.items():                          # (Adam reads the gradient buffer, it does not write it)
        g = ts.grad[off:off + n].cpu().double().numpy()
        gr = chk["grads"][name].reshape(-1).numpy()
        e = np.linalg.norm(g - gr) / max(np.linalg.norm(gr), 1e-12)
        if e > GRAD_TOL:
            bad.append((name, e))
    assert not bad, bad
    assert ts.step_count == 1


@pytest.mark.parametrize("name,space,bins,option", [("vo_cnn_wider", ["rgb", "depth"], 0, None),
                                                    ("vo_cnn_rgb_d_dd_top_down", SPACE, 10, ("wgrad_stem", "fp32"))])
def test_handles_off_the_frame_kernels_take_the_pair_path_with_equal_results(name, space, bins, option):
    """Fallback: the pairs are materialised into a workspace and the pair path runs — forward_backward_raw equals forward_backward on
    the built pairs, running statistics included (fresh copies of the same model)."""
    H, W, B = 37, 45, 2
    rgb, dep = frames(B, H, W, seed=17)
    obs = materialise(rgb, dep, H, W, bins, want_tdv="top_down_view" in space)
    target = torch.from_numpy(synth.uniform(7, "tgt", (B, 3), -0.3, 0.3).astype(np.float32)).to(DEV)
    res = []
    for form in ("pairs", "frames"):
        model = build_model(name, space, W, H, seed=8, bins=bins)
        ts = VOTrainStep(model)
        if option:
            model.set_option(*option)
        if form == "pairs":
            out, loss = ts.forward_backward({k: v for k, v in obs.items() if k in space}, target=target)
        else:
            out, loss = ts.forward_backward_raw(rgb, dep, obs.get("top_down_view"), target=target)
        torch.cuda.synchronize()
        rmv = model.visual_encoder.running_mean_and_var
        res.append((out.clone(), ts.grad.clone(), loss.clone(), rmv._mean.clone(), rmv._var.clone(), rmv._count.clone()))
    for a, b in zip(*res):
        assert torch.isfinite(a).all() and torch.equal(a, b)


def test_forward_train_raw_returns_without_waiting_for_the_stream():
    """A backlog is queued on the stream with an event behind it; when forward_train_raw returns the event must still be pending."""
    H, W, B = 66, 98, 3
    model = build_model("vo_cnn_rgb_d_dd_top_down", SPACE, W, H, seed=4)
    ts = VOTrainStep(model)
    rgb, dep = frames(B, H, W, seed=11)
    obs = materialise(rgb, dep, H, W, 10)
    a = torch.randn((4096, 4096), device=DEV)
    b = torch.empty_like(a)
    for _ in range(2):                                # warm-up: workspaces, the matmul's own set-up
        ts.forward_train_raw(rgb, dep, obs["top_down_view"])
        ts.forward_train(obs)
        torch.mm(a, a, out=b)
    torch.cuda.synchronize()

    def pending_after(fn):
        for _ in range(300):                          # some hundred milliseconds of queued work
            torch.mm(a, a, out=b)
        ev = torch.cuda.Event()
        ev.record()
        fn()
        done = ev.query()
        torch.cuda.synchronize()
        return not done

    assert pending_after(lambda: None), "the backlog is too short to show anything"
    assert pending_after(lambda: ts.forward_train_raw(rgb, dep, obs["top_down_view"]))
    print("forward_train (pairs) returned with the backlog still pending:", pending_after(lambda: ts.forward_train(obs)))


def test_geo_invariance_step_takes_a_frame_batch():
    """inverse_joint_train, left and right models, 45x37, 8 entries: a frame batch against the pair batch built from it (fresh copies
    of the same models).  The running statistics differ by the moments' last ulp, so preds and total are held to the `out` bounds of
    the fp64 comparison (rtol 2e-4 / atol 2e-5)."""
    H, W, P = 37, 45, 4
    rgb, dep = frames(P, H, W, seed=19)
    rgb = torch.stack([x for i in range(P) for x in (rgb[i], rgb[i].flip(0))]).contiguous()          # entry 2i + 1: (cur, prev)
    dep = torch.stack([x for i in range(P) for x in (dep[i], dep[i].flip(0))]).contiguous()
    obs = materialise(rgb, dep, H, W, 10)
    acts = (synth.bits(19, "acts", P) % np.uint64(2)).astype(np.int64) + 2
    actions = np.stack([x for i in range(P) for x in (acts[i], 5 - acts[i])])
    dtypes = np.tile(np.array([0, 1], dtype=np.int64), P)
    targets = synth.uniform(19, "tgt", (2 * P, 3), -0.3, 0.3).astype(np.float32)
    res = []
    for form in ("pairs", "frames"):
        steps = {a: VOTrainStep(build_model("vo_cnn_rgb_d_dd_top_down", SPACE, W, H, seed=20 + a)) for a in (2, 3)}
        js = GeoInvarianceTrainStep(steps, ("inverse_joint_train",), loss_inv_weight=1.0)
        batch = obs if form == "pairs" else {"rgb_frames": rgb, "depth_frames": dep, "top_down_view": obs["top_down_view"]}
        total, preds = js.step(batch, actions, dtypes, targets)
        torch.cuda.synchronize()
        res.append((total.cpu().numpy(), preds.cpu().numpy(), {a: st.step_count for a, st in steps.items()}))
    assert res[0][2] == res[1][2] == {2: 1, 3: 1}
    assert np.isfinite(res[1][1]).all()
    np.testing.assert_allclose(res[1][1], res[0][1], rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(res[1][0], res[0][0], rtol=2e-4, atol=2e-5)


def test_batcher_frames_reproduce_the_pair_batch():
    """process_chunk(frames=True) against process_chunk() on the same chunk, swapped entries included: the frames re-assembled into
    pairs with the batcher's edges are the pair tensors, the top-down pairs and the bookkeeping are identical."""
    W, H = 64, 48
    infos = dict(min_depth=0.1, max_depth=10.0, vis_size_h=H, vis_size_w=W, hfov_rad=np.deg2rad(70.0), rows_around_center=9)
    ch = synth.make_dataset_chunk(10, H, W, seed=51)
    b = StatePairBatcher(W, H, act_type=[2, 3], discretize_depth="hard", discretized_depth_channels=10, gen_top_down_view=True,
                         top_down_view_infos=infos, geo_invariance_types=("inverse_joint_train",))
    pairs, frm = b.process_chunk(ch, chunk_i=3), b.process_chunk(ch, chunk_i=3, frames=True)
    torch.cuda.synchronize()
    M = pairs["rgb_pairs"].shape[0]
    assert M > 0 and bool((pairs["data_types"] == 1).any())            # swapped entries are there
    obs_keys = {"rgb_pairs", "depth_pairs", "discretized_depth_pairs", "top_down_view_pairs"}
    assert set(frm) == (set(pairs) - obs_keys) | {"rgb_frames", "depth_frames", "top_down_view_pairs", "edges"}
    for k in set(pairs) - obs_keys:
        assert torch.equal(pairs[k], frm[k]), k
    assert frm["rgb_frames"].dtype == torch.uint8 and tuple(frm["rgb_frames"].shape) == (M, 2, H, W, 3)
    assert frm["depth_frames"].dtype == torch.float32 and tuple(frm["depth_frames"].shape) == (M, 2, H, W)
    assert list(frm["edges"]) == list(b.edges) and [float(x) for x in frm["edges"]] == E16.tolist()
    assert torch.equal(frm["rgb_frames"].permute(0, 2, 3, 1, 4).reshape(M, H, W, 6).float(), pairs["rgb_pairs"])
    assert torch.equal(frm["depth_frames"].permute(0, 2, 3, 1).contiguous(), pairs["depth_pairs"])
    assert torch.equal(onehot(frm["depth_frames"], list(frm["edges"])), pairs["discretized_depth_pairs"])
    assert torch.equal(frm["top_down_view_pairs"], pairs["top_down_view_pairs"])
