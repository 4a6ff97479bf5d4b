"""GPU (-m gpu): one training step of the model variants the other training tests do not reach — the 64-base-plane models
(vo_cnn_wider, vo_cnn_wider_act_embed) and the five modality subsets (vo_cnn_rgb, vo_cnn_rgb_d_top_down, vo_cnn_d_dd_top_down,
vo_cnn_rgb_d_dd, vo_cnn_rgb_dd_top_down) — against the fp64 checker (oracle/torch_train_ref.py, itself pinned to the reference on
the wider and the rgb + one-hot + top-down shapes by tests/test_train_ref_golden.py).

Why these: a 64-output stem is not served by the matrix-core stem weight-gradient kernel nor by the planner's STEM_LDS branch, so
its weight gradient runs on `generic tg7 mode2`, which no other GPU test reaches; stages of 64 .. 512 channels give the x3, mw12,
lds9 and generic plans pairs = 256, where their `256 / pairs`, `512 / pairs` and `2048 / pairs` chunk quotients reach 1 or 2 (the default
model stops at pairs = 64); and the stem's weight gradient reads the
observation tensors through per-model channel tables, which the forward parity fixtures (outputs only) cannot check.

Each step: train mode, dropout 0, normalize_visual_inputs=True, 45x37 (maps 19x23, 10x12, 5x6, 3x3, 2x2: odd maps under every
stride-2 conv, ragged tiles) with 3 pairs, and the wider model once at 98x66 with 2 pairs (first stage 17x25: two 16-wide strips,
the second ragged, several row segments).  Weights, inputs and targets are seeded (seed 51: the two fixtures' seed).

    output, loss, buffers   the bounds of tests/test_gpu_train.py::test_train_step_matches_reference
    every gradient          rel L2 <= 3 d32 + 2e-6, d32 = the float32 checker's rel L2 against its float64 self on the same inputs
                            (test_full_resolution_gradients_against_the_fp64_checker's criterion)
    conv1.0.weight          the same per INPUT CHANNEL, on the slice [:, c] with d32 of that slice: one swapped or dropped channel
                            is invisible in the tensor's norm
    the checker itself      d32 <= 1e-5 for every tensor and every stem slice of every case (asserted; a CPU statement about the
                            seeds): the bound then stays below 3.2e-5, tests/test_gpu_train.py's GRAD_TOL, and no ReLU mask of the
                            float32 checker flips
    after optimizer_step    (wider, rgb + one-hot + top-down) the eval forward against oracle.forward on the checker's new parameters:
                            the device-side re-pack of a 64-channel stem and of the one-hot tables
    coverage                test_the_cases_reach_the_kernels_they_are_meant_to asks pnvo_wgrad_describe for every weight-gradient
                            request of every case's backward

The modality models run three stem selections.  Under wgrad_stem=fp32 only the stem's weight gradient changes kernel; adding
wgrad=generic also moves the three stride-2 3x3 convs from the twelve-wave kernel to the generic one.  Tensors whose request is
planned as in the default run must equal that run bit for bit; the others are held to the fp64 criterion.

Measured on the MI355X (the tensor closest to its bound: err / d32;  median err;  the stem's input channel closest to its bound:
err / d32 of the slice).  The wgrad3 / wgrad / pool_bwd options do not touch the tensor closest to its bound (a GroupNorm bias):
    wider {}, wgrad3=fp32, +wgrad=lds9, +wgrad=generic, pool_bwd=separate
                                 layer1.0.convs.1.bias 1.7e-6 / 2.1e-6;    1.3e-6;  channel 6: 1.7e-6 / 2.3e-6
    wider conv=x3                layer2.1.convs.1.bias 1.9e-6 / 2.1e-6;    1.5e-6;  channel 6: 1.8e-6 / 2.3e-6
    wider conv=x3 train_pieces=3 layer1.0.convs.4.weight 2.7e-6 / 2.5e-6;  1.9e-6;  channel 2: 2.3e-6 / 2.5e-6
    wider 98x66                  layer1.0.convs.4.weight 1.8e-6 / 2.9e-6;  1.5e-6;  channel 0: 1.5e-6 / 3.2e-6
    wider_act_embed              layer1.1.convs.1.weight 2.3e-6 / 2.6e-6;  1.9e-6;  channel 7: 2.1e-6 / 3.0e-6
    rgb                          layer2.0.convs.1.weight 1.9e-6 / 2.7e-6;  1.2e-6;  channel 0: 1.5e-6 / 2.7e-6
    rgb_d_top_down               layer1.0.convs.1.weight 1.6e-6 / 1.7e-6;  1.2e-6;  channel 0: 1.5e-6 / 2.1e-6
    d_dd_top_down                layer1.0.convs.1.bias 1.8e-6 / 2.2e-6;    1.1e-6;  channel 3: 1.4e-6 / 2.2e-6
    rgb_d_dd                     layer2.0.convs.4.weight 1.5e-6 / 1.7e-6;  1.1e-6;  channel 3: 1.4e-6 / 1.9e-6
    rgb_dd_top_down              layer1.0.convs.1.bias 2.0e-6 / 1.8e-6;    9.7e-7;  channel 21: 1.5e-6 / 2.4e-6
    wgrad_stem=fp32 (five models)            conv1.0.weight 1.3e-6 .. 1.5e-6 / 2.0e-6 .. 2.6e-6;  worst channel 1.5e-6 / 2.1e-6
    wgrad_stem=fp32 wgrad=generic (five)     the four re-planned tensors 1.3e-6 .. 1.7e-6 / 2.0e-6 .. 2.7e-6;  worst channel 1.6e-6 / 2.5e-6
Largest d32 of any tensor or stem slice over the eight (model, size) cases: 5.1e-6 (wider 98x66, layer1.0.convs.0.weight).
Wall time of the module on the MI355X host (16 CPUs): 7.4 s, the checker's float64 and float32 steps included (each of the 25 tests
below 1.3 s).
"""
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch

from conftest import golden_case, load_golden
from oracle import oracle
from oracle import torch_train_ref as ref
from pointnav_vo_amd import model_spec as ms, synth
from pointnav_vo_amd.registry import baseline_registry
from pointnav_vo_amd import vo_cnn  # noqa: F401
from pointnav_vo_amd.train import VOTrainStep

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import gen_golden_wgrad_bits as gwb  # noqa: E402  (the weight-gradient requests of a backward, described by the planner)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEM = "visual_encoder.backbone.conv1.0.weight"
RMV = "visual_encoder.running_mean_and_var."
DD, TDV = "discretized_depth", "top_down_view"
SEED = 51
D32_MAX = 1e-5          # the float32 checker against its float64 self: beyond it the 3 d32 bound stops checking much

# key -> model, observation space, one-hot bins, W, H, pairs, actions, reference-captured fixture
CASES = {
    "wider": ("vo_cnn_wider", ["rgb", "depth"], 0, 45, 37, 3, None, "train_wider_45x37_b3_f64.npz"),
    "wider98": ("vo_cnn_wider", ["rgb", "depth"], 0, 98, 66, 2, None, None),
    "wider_act": ("vo_cnn_wider_act_embed", ["rgb", "depth"], 0, 45, 37, 3, (1, 3, 1), None),
    "rgb": ("vo_cnn_rgb", ["rgb"], 0, 45, 37, 3, None, None),
    "rgb_d_tdv": ("vo_cnn_rgb_d_top_down", ["rgb", "depth", TDV], 0, 45, 37, 3, None, None),
    "d_dd_tdv": ("vo_cnn_d_dd_top_down", ["depth", DD, TDV], 10, 45, 37, 3, None, None),
    "rgb_d_dd": ("vo_cnn_rgb_d_dd", ["rgb", "depth", DD], 10, 45, 37, 3, None, None),
    "rgb_dd_tdv": ("vo_cnn_rgb_dd_top_down", ["rgb", DD, TDV], 10, 45, 37, 3, None, "train_rgb_dd_tdv_45x37_b3_f64.npz"),
}
WIDER_OPTS = [{}, {"wgrad3": "fp32"}, {"wgrad3": "fp32", "wgrad": "lds9"}, {"wgrad3": "fp32", "wgrad": "generic"}, {"conv": "x3"},
              {"conv": "x3", "train_pieces": "3"}, {"pool_bwd": "separate"}]
SUBSETS = ["rgb", "rgb_d_tdv", "d_dd_tdv", "rgb_d_dd", "rgb_dd_tdv"]
STEM_OPTS = [{"wgrad_stem": "fp32"}, {"wgrad_stem": "fp32", "wgrad": "generic"}]
# every (case, options) a test of this module runs: what the coverage test describes
RUNS = ([("wider", o) for o in WIDER_OPTS] + [("wider98", {}), ("wider_act", {})] +
        [(k, o) for k in SUBSETS for o in [{}] + STEM_OPTS])


def opt_id(o):
    return ",".join(f"{k}={v}" for k, v in o.items()) or "default"


def rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@functools.lru_cache(maxsize=None)
def checker(key):
    """Weights, inputs and target of a case, the checker's float64 step on them, and d32: the float32 checker's relative L2 against
    it, per tensor and per input channel of the stem weight.  Computed once and left unchanged."""
    name, space, bins, W, H, B, actions, fixture = CASES[key]
    if fixture:
        rec = load_golden(fixture)
        assert (str(rec["model"]), str(rec["obs_space"]).split(","), int(rec["width"]), int(rec["height"]), int(rec["batch"]),
                int(rec["dd_bins"]), int(rec["seed"])) == (name, space, W, H, B, bins, SEED)
        cfg, sd, obs, _ = golden_case(rec)
        target = rec["target"]
    else:
        cfg = ms.config_from_kwargs(observation_space=space, observation_size=(W, H), hidden_size=512, normalize_visual_inputs=True,
                                    resnet_baseplanes=64 if "wider" in name else 32, output_dim=3, discretized_depth_channels=bins,
                                    act_embed=actions is not None)
        sd = synth.make_state_dict(ms.state_dict_spec(cfg), seed=SEED)
        obs = synth.make_obs_pairs(B, H, W, observation_space=space, dd_bins=max(bins, 1), seed=SEED)
        target = synth.uniform(SEED, "train_target", (B, 3), -0.3, 0.3).astype(np.float32)
    acts = None if actions is None else np.asarray(actions, dtype=np.int64)
    c64 = ref.train_step(sd, obs, target, ngroups=cfg.ngroups, dtype=torch.float64, actions=acts)
    c32 = ref.train_step(sd, obs, target, ngroups=cfg.ngroups, dtype=torch.float32, actions=acts)
    g64 = {k: v.numpy() for k, v in c64["grads"].items()}
    g32 = {k: v.double().numpy() for k, v in c32["grads"].items()}
    d32 = {k: rel(g32[k], g64[k]) for k in g64}
    stem_d32 = np.array([rel(g32[STEM][:, c], g64[STEM][:, c]) for c in range(g64[STEM].shape[1])])
    emb_d32 = None
    if acts is not None:
        e = "action_embedding.weight"
        emb_d32 = np.array([rel(g32[e][r], g64[e][r]) if r in acts else 0.0 for r in range(g64[e].shape[0])])
    return types.SimpleNamespace(key=key, name=name, space=space, bins=bins, W=W, H=H, B=B, actions=acts, cfg=cfg, sd=sd, obs=obs,
                                 target=target, c64=c64, g64=g64, d32=d32, stem_d32=stem_d32, emb_d32=emb_d32)


def assert_the_checker_is_float32_stable(c):
    """The condition under which `3 d32 + 2e-6` is a float32-grade bound: it concerns the checker and the seeds only."""
    worst = max(c.d32, key=c.d32.get)
    assert c.d32[worst] <= D32_MAX, (c.key, worst, c.d32[worst])
    assert c.stem_d32.max() <= D32_MAX, (c.key, "stem input channel", int(c.stem_d32.argmax()), c.stem_d32.max())
    assert c.g64[STEM].shape[1] == c.cfg.in_channels and all(np.linalg.norm(c.g64[STEM][:, ch]) > 0 for ch in range(c.cfg.in_channels))
    if c.bins:        # every one-hot bin of both frames occurs: no input channel's gradient is degenerate
        assert c.obs[DD].shape[-1] == 2 * c.bins and (c.obs[DD].reshape(-1, 2 * c.bins).sum(0) > 0).all()


def hip_step(key, opts):
    """One train-mode forward_backward of a fresh model under `opts` -> (model, step object, device inputs, out, loss, gradients by
    name as float64 arrays of the parameters' shapes)."""
    c = checker(key)
    kw = dict(observation_space=c.space, observation_size=(c.W, c.H), hidden_size=512, backbone="resnet18", normalize_visual_inputs=True,
              output_dim=3, dropout_p=0.0)
    if c.bins:
        kw["discretized_depth_channels"] = c.bins
    model = baseline_registry.get_vo_model(c.name)(**kw)
    assert model.cfg == c.cfg
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in c.sd.items()})
    model = model.to(DEV)
    for k, v in opts.items():
        model.set_option(k, v)
    ts = VOTrainStep(model)
    tobs = {k: torch.from_numpy(v).to(DEV) for k, v in c.obs.items()}
    out, loss = ts.forward_backward(tobs, target=torch.from_numpy(c.target).to(DEV),
                                    actions=None if c.actions is None else torch.from_numpy(c.actions))
    torch.cuda.synchronize()
    flat = ts.grad.cpu().double().numpy()
    assert set(ts.offsets) == set(c.g64)
    grads = {n: flat[o:o + k].reshape(c.g64[n].shape) for n, (o, k) in ts.offsets.items()}
    return model, ts, tobs, out, loss, grads


def check_forward(c, model, out, loss):
    """Output, loss and the RunningMeanAndVar buffers: the bounds of test_gpu_train.py::test_train_step_matches_reference."""
    np.testing.assert_allclose(out.cpu().numpy(), c.c64["out"].numpy(), rtol=2e-4, atol=2e-5)
    want = float(c.c64["loss"])
    assert abs(loss.item() - want) < 1e-4 * max(1.0, abs(want)), (loss.item(), want)
    for k in ("_mean", "_var", "_count"):
        b = getattr(model.visual_encoder.running_mean_and_var, k).cpu().double().numpy().reshape(-1)
        np.testing.assert_allclose(b, c.c64["buffers"][RMV + k].numpy().reshape(-1), rtol=1e-5, atol=1e-6, err_msg=k)


def check_gradients(c, grads, opts, names=None):
    """rel L2 <= 3 d32 + 2e-6 for the tensors `names` (default: all), and per input channel of the stem weight."""
    rows, bad = [], []
    for n in names if names is not None else list(c.g64):
        err = rel(grads[n], c.g64[n])
        rows.append((n, err, c.d32[n]))
        if not err <= 3.0 * c.d32[n] + 2e-6:
            bad.append((n, err, c.d32[n]))
    srows = []
    if names is None or STEM in names:
        for ch in range(c.g64[STEM].shape[1]):
            err = rel(grads[STEM][:, ch], c.g64[STEM][:, ch])
            d = float(c.stem_d32[ch])
            srows.append((ch, err, d))
            if not err <= 3.0 * d + 2e-6:
                bad.append((f"{STEM}[:, {ch}]", err, d))
    close = lambda r: r[1] / (3.0 * r[2] + 2e-6)
    w = max(rows, key=close)
    line = f"{c.key} {opt_id(opts)}: closest to its bound {w[0]} {w[1]:.1e} / {w[2]:.1e}; median err {np.median([r[1] for r in rows]):.1e}"
    if srows:
        s = max(srows, key=close)
        line += f"; stem input channel {s[0]}: {s[1]:.1e} / {s[2]:.1e}"
    print(line)
    assert not bad, bad


def check_eval_after_the_step(c, model, ts, tobs):
    """optimizer_step, then the eval forward (operands re-packed on the device) against the checker's new parameters."""
    before = ts.flat.clone()
    ts.optimizer_step()
    torch.cuda.synchronize()
    assert not torch.equal(before, ts.flat)
    newsd = {**{k: v.numpy() for k, v in c.c64["params"].items()}, **{k: v.numpy() for k, v in c.c64["buffers"].items()}}
    want = oracle.forward(newsd, c.obs, ngroups=c.cfg.ngroups, dtype=np.float64)
    with torch.no_grad():
        got = model.eval()(tobs).cpu().numpy()
    err = np.linalg.norm(got - want, axis=1) / np.maximum(np.linalg.norm(want, axis=1), 1e-2)
    assert err.max() < 5e-3, err          # parameters differ by <= 2 lr where the gradient sign was ambiguous


@functools.lru_cache(maxsize=None)
def wider_default_gradients():
    return hip_step("wider", {})[5]


@pytest.mark.parametrize("opts", WIDER_OPTS, ids=opt_id)
def test_wider_step_matches_the_fp64_checker(opts):
    """vo_cnn_wider at 45x37, 3 pairs (odd batch): the generic observation-fetch stem weight gradient, the fused (or, last case,
    separate) max-pool backward at 64 channels, 64 .. 512-channel stages under each weight-gradient family and conv family."""
    c = checker("wider")
    assert_the_checker_is_float32_stable(c)
    model, ts, tobs, out, loss, grads = hip_step("wider", opts)
    check_forward(c, model, out, loss)
    check_gradients(c, grads, opts)
    if not opts:
        check_eval_after_the_step(c, model, ts, tobs)
    elif "pool_bwd" not in opts:      # another kernel family somewhere: float32-grade, not bit, equal (equal would mean the options selected nothing)
        base = wider_default_gradients()
        assert any(not np.array_equal(grads[n], base[n]) for n in grads), opts


def test_wider_step_at_98x66_matches_the_fp64_checker():
    """First stage 17x25: two 16-wide strips of the matrix-core weight-gradient kernel, the second ragged, several row segments."""
    c = checker("wider98")
    assert_the_checker_is_float32_stable(c)
    assert c.cfg.layer_hw(1) == (17, 25)
    model, ts, tobs, out, loss, grads = hip_step("wider98", {})
    check_forward(c, model, out, loss)
    check_gradients(c, grads, {})


def test_wider_act_embed_step_matches_the_fp64_checker():
    """vo_cnn_wider_act_embed, actions [1, 3, 1]: as above, plus the embedding rows — rows of unused actions exactly zero, the row used
    twice the sum of both samples' gradients (each used row against fp64 with the module's criterion)."""
    c = checker("wider_act")
    assert_the_checker_is_float32_stable(c)
    assert c.emb_d32.max() <= D32_MAX, c.emb_d32
    model, ts, tobs, out, loss, grads = hip_step("wider_act", {})
    check_forward(c, model, out, loss)
    check_gradients(c, grads, {})
    emb, want = grads["action_embedding.weight"], c.g64["action_embedding.weight"]
    used = sorted(set(c.actions.tolist()))
    assert used == [1, 3] and list(c.actions).count(1) == 2
    for r in range(emb.shape[0]):
        if r in used:
            assert emb[r].any() and rel(emb[r], want[r]) <= 3.0 * c.emb_d32[r] + 2e-6, (r, rel(emb[r], want[r]), c.emb_d32[r])
        else:
            assert not emb[r].any() and not want[r].any(), r


@functools.lru_cache(maxsize=None)
def subset_default_run(key):
    """The default step of a modality model: checked against fp64 by test_modality_subset_step_matches_the_fp64_checker, and the
    bit-for-bit baseline of the other stem selections.  -> (model, step object, device inputs, then on the host: out, loss, gradients)."""
    model, ts, tobs, out, loss, grads = hip_step(key, {})
    return model, ts, tobs, out.cpu(), loss.cpu(), grads


@pytest.mark.parametrize("key", SUBSETS)
def test_modality_subset_step_matches_the_fp64_checker(key):
    """Default options: the stem's weight gradient on the bf16 matrix cores, through the model's own slot maps."""
    c = checker(key)
    assert_the_checker_is_float32_stable(c)
    model, ts, tobs, out, loss, grads = subset_default_run(key)
    check_forward(c, model, out, loss)
    check_gradients(c, grads, {})
    if key == "rgb_dd_tdv":          # (the other tests use the cached run's host copies only, not its model)
        check_eval_after_the_step(c, model, ts, tobs)


def planned(c, opts):
    """parameter name -> describe line of its weight-gradient request under `opts` (the stem only where the planner serves it)."""
    seen = []
    gwb.describe_requests(seen, c.cfg, c.B, opts, dropout=False)
    names = gwb.request_names(c.cfg, opts)
    assert len(names) == len(seen)
    return {n: text for n, (text, _) in zip(names, seen)}


@pytest.mark.parametrize("opts", STEM_OPTS, ids=opt_id)
@pytest.mark.parametrize("key", SUBSETS)
def test_modality_subset_stem_selections(key, opts):
    """wgrad_stem=fp32: the float32 LDS stem kernel reading the observation tensors through the whitening and channel tables;
    with wgrad=generic: the generic kernel's observation fetch.  conv1.0.weight, whole and per input channel, and every tensor
    whose request is planned otherwise than in the default run against fp64; everything else bit for bit against the default run."""
    c = checker(key)
    assert_the_checker_is_float32_stable(c)
    base_out, base_loss, base = subset_default_run(key)[3:]
    model, ts, tobs, out, loss, grads = hip_step(key, opts)
    assert torch.equal(out.cpu(), base_out) and torch.equal(loss.cpu(), base_loss)      # the forward does not depend on these options
    was, now = planned(c, {}), planned(c, opts)
    moved = [n for n in now if now[n] != was.get(n)]
    assert STEM in moved and STEM not in was
    assert len(moved) == (1 if "wgrad" not in opts else 4), moved                       # + the three stride-2 3x3 convs
    assert not np.array_equal(grads[STEM], base[STEM])                                  # (equal would mean the option selected nothing)
    check_gradients(c, grads, opts, names=moved)
    for n in c.g64:
        if n not in moved:
            assert np.array_equal(grads[n], base[n]), n


def test_the_cases_reach_the_kernels_they_are_meant_to():
    """pnvo_wgrad_describe on every weight-gradient request of every run of this module (RUNS: what the tests above parametrise over)."""
    seen = []          # (instance name, problem as a dict, case key)
    for key, opts in RUNS:
        c = checker(key)
        got = []
        gwb.describe_requests(got, c.cfg, c.B, opts, dropout=False)
        seen += [(text.split(" | ")[0], dict(zip(gwb.FIELDS, row)), text, key) for text, row in got]
    geometry = lambda text: text.split(" | ")[2].split(" ppc ")[0].split("ci_tiles ")[1]          # "<n> pairs <n> chunks <n>"
    for line in sorted({f"{inst:18s} B {q['B']} {q['CIN']:3d} -> {q['COUT']:3d} {q['Ho']:2d}x{q['Wo']:<2d} k{q['KH']} s{q['stride']} np{q['np']} "
                        f"| ci_tiles {geometry(text)}" for inst, q, text, _ in seen}):
        print("request:", line)
    stems = [(inst, q, key) for inst, q, _, key in seen if q["mode"] == 2]
    # the 64-output stem: neither the matrix-core stem kernel nor STEM_LDS (`q.COUT == 32`) takes it
    assert any(inst == "generic tg7 mode2" and q["COUT"] == 64 for inst, q, _ in stems), stems
    # a 32-output stem under wgrad_stem=fp32 + wgrad=generic
    assert any(inst == "generic tg7 mode2" and q["COUT"] == 32 and q["wgrad"] == 2 for inst, q, _ in stems), stems
    # STEM_LDS on a model with fewer than 32 input channels (the request itself always says CIN = 32, one padded tile: wgrad_request)
    assert any(inst == "stem_lds" and checker(key).cfg.in_channels < 32 for inst, q, key in stems), stems
    assert {checker(key).cfg.in_channels for inst, _, key in stems if inst == "stem_lds"} == {6, 10, 24, 28}
    # 512 -> 512 channels, pairs = 256, in each 3x3 family (none of the four planners refuses it)
    for fam in ("x3", "mw12", "lds9", "generic tg9"):
        hit = [text for inst, q, text, _ in seen if inst.startswith(fam + " ") and q["CIN"] == 512 and q["COUT"] == 512]
        assert hit and all(" pairs 256 " in t for t in hit), (fam, hit)
