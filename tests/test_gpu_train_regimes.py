"""GPU (-m gpu): the default training step at 341x192 (VOTrainStep, normalize_visual_inputs=True, dropout 0.2) against the fp64
checker AT ITS REAL BATCH — 4, 8, 33, 34, 128 and 208 pairs — with every default kernel selection of that batch: the split
matrix-core weight-gradient kernels from 112 workgroups on (not at 4 pairs, yes at 8), an odd batch and its even neighbour, configs[3]'s 128 pairs
exactly as bench.py --config train sets them up (bench.make_inputs(128, dev, 0), weights of seed 0, the bench's target
generator) and 208 pairs, where the forward takes the eight-wave deep-stage forms.  RunningMeanAndVar's update and dropout's
masks are part of the step: the HIP step's own masks are read back (pnvo_train_dropout_mask) and handed to the checker.

Checker: oracle/torch_train_ref.train_step_chunked (16 pairs per autograd graph; exact, tests/test_train_ref_chunked.py), run in
float64 and in float32.  Per step:
    loss                 within 1e-5 relative of fp64
    every gradient       rel L2 <= 3 d32 + 2e-6, d32 = the float32 checker's rel L2 against fp64 on the same batch
                         (the criterion of test_full_resolution_gradients_against_the_fp64_checker)
    running statistics   mean / var within 1e-5 relative (float32-grade), count exact
    one Adam step        no element further than 2 lr from the checker's parameters; the fraction of elements more than
                         0.1 lr off the checker's path below OFF_TOL
Measured on the MI355X (the tensor closest to its bound: err / d32; median err / median d32; Adam: worst distance, share off path):
    B = 4     layer3.0.convs.1.bias 1.5e-6 / 2.4e-6;  1.3e-6 / 3.0e-6;  0.85 lr, 0.00 %
    B = 8     visual_fc.2.weight    6.6e-7 / 1.6e-6;  1.2e-6 / 1.4e-2;  2.00 lr, 0.00 %
    B = 33    layer4.1.convs.1.bias 8.2e-4 / 1.3e-6 (ten tensors, one near-zero flip: see below);  3.7e-4 / 1.0e-3;  2.00 lr, 0.01 %
    B = 34    layer4.1.convs.4.bias 2.1e-4 / 9.0e-7 (three tensors, one near-zero flip);  3.0e-4 / 7.9e-4;  2.00 lr, 0.00 %
    B = 128   layer2.0.downsample.1.weight 1.4e-3 / 2.7e-3;  1.4e-4 / 8.9e-4;  2.00 lr, 0.00 %
    B = 208   layer4.0.downsample.1.weight 1.7e-4 / 1.8e-4;  5.0e-4 / 8.8e-4;  2.00 lr, 0.01 %
OFF_TOL = 1e-3: ten times the largest share measured.
What the bounds are worth.  d32 depends on the batch and its inputs: on these inputs the median d32 is 3e-6 at 4 pairs but 1.4e-2
at 8 (the float32 checker flips ReLU masks in the early layers), so at such batches the gradient bound admits errors of several
percent on many tensors and checks little there; it is tight where the checker's own float32 run flips nothing (layer4 and
behind at 33 pairs: 1e-6).  On a first Adam step every element moves by about lr whatever its gradient, so "within 2 lr" always
holds (it is met at 2.00 lr); the check that bites is the share of elements off the checker's path.
One near-zero flip.  Where an fp64 ReLU input lies within float32 rounding of zero (|x| / rms < FLIP_TOL = 2e-6; the forward's
float32-grade error is 1.6e-6 of the feature norm, tests/test_gpu_batch_regimes.py) the sign, and so the mask, is not defined
at float32 precision, and one such mask decides a gradient path: a single flip moves the tensors behind it by ~1e-3 of their
norm, far beyond a d32 of 1e-6 when the float32 checker happens to flip nothing there.  So when tensors fail, the test looks
for ONE such element (in the ReLUs at or behind the failing tensors) whose flip in the fp64 reference brings every tensor within
3 d32 + 2e-6, and fails if there is none.  Measured: 33 pairs fail ten layer4 tensors (worst layer4.1.convs.1.bias 8.2e-4 where
d32 is 1.3e-6); flipping pair 10's element of layer4.1's first ReLU, fp64 input -3.7e-7 (3.5e-7 of the rms), brings all within
(worst 0.73 of the bound).  34 pairs fail three layer4 tensors in the same way (explained by pair 33's element of layer4.1's output ReLU, 1.6e-7 of the
rms), 32 none: it is not tied to odd batches.  The
three-piece training forward (train_pieces=3) passes 33 pairs without a flip: its three bf16 pieces round differently.
Wall time of the module on the MI355X host (16 CPUs): 64 s, the chunked checker in float64 and float32 included."""
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import oracle
from oracle import torch_train_ref as ref
from pointnav_vo_amd import model_spec as ms, synth
from pointnav_vo_amd.registry import baseline_registry
from pointnav_vo_amd import vo_cnn  # noqa: F401
from pointnav_vo_amd.train import VOTrainStep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the bench's device-side inputs)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
RMV = "visual_encoder.running_mean_and_var."
OFF_TOL = 1e-3
FLIP_TOL = 2e-6        # |x| / rms of a ReLU input below which float32-grade forwards may disagree on its sign


def setup(B):
    """(model, sd, obs on the device, target on the device) — for 128 pairs exactly tools/bench_configs.run_train's."""
    seed = 0 if B == 128 else 3
    model = baseline_registry.get_vo_model("vo_cnn_rgb_d_dd_top_down")(
        observation_space=bench.SPACE, observation_size=(bench.W, bench.H), hidden_size=512, backbone="resnet18",
        normalize_visual_inputs=True, output_dim=3, dropout_p=0.2, discretized_depth_channels=bench.BINS)
    sd = synth.make_state_dict(ms.state_dict_spec(model.cfg), seed=seed)
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    model = model.to(DEV)
    obs = bench.make_inputs(B, DEV, 0 if B == 128 else B)
    g = torch.Generator(device=DEV)
    g.manual_seed(7 if B == 128 else 100 + B)
    tgt = (torch.rand((B, 3), device=DEV, generator=g) - 0.5) * 0.5
    return model, sd, obs, tgt


class _Relu:
    """The checker's ReLU that records, per call in forward order, the elements of its input within FLIP_TOL of zero (relative
    to the input's rms), or flips the mask of one element of one call (the value there is within rounding of zero either way)."""

    def __init__(self, flip=None):
        self.call, self.flip, self.near = 0, flip, []

    def __call__(self, x):
        call = self.call
        self.call += 1
        if self.flip is None:
            rel = (x.detach().abs() / x.detach().pow(2).mean().sqrt()).reshape(-1)
            idx = torch.nonzero(rel < FLIP_TOL).reshape(-1)
            self.near += [(float(rel[i]), call, int(i)) for i in idx]
            return F.relu(x)
        if self.flip[0] != call:
            return F.relu(x)
        m = (x.detach() > 0).to(x.dtype).reshape(-1).clone()
        m[self.flip[1]] = 1.0 - m[self.flip[1]]
        return x * m.reshape(x.shape)


def sample_grads(sd, host, target, masks, buffers, ngroups, B, s, relu):
    """fp64 gradient contribution of pair s to the mean loss over B pairs, whitening fixed to `buffers`, with ReLU `relu`."""
    params = {k: torch.as_tensor(v).double().clone().requires_grad_(True) for k, v in sd.items()
              if k.rsplit(".", 1)[-1] not in ("_mean", "_var", "_count")}
    out, _ = ref.forward(params, buffers, {k: torch.as_tensor(v[s:s + 1]) for k, v in host.items()}, ngroups=ngroups, train=False,
                         dtype=torch.float64, drop_masks=tuple(m[s:s + 1] for m in masks), relu=relu)
    (ref.regression_loss(out, torch.as_tensor(target[s:s + 1]).double()) * (1.0 / B)).backward()
    return {k: p.grad.detach() for k, p in params.items()}


def first_relu(name):
    """Index, in forward order, of the first ReLU behind the parameter `name` (stem 0; two per BasicBlock; compression 17; hidden 18)."""
    m = re.search(r"layer(\d)\.(\d)\.", name)
    if m:
        return 1 + 2 * (2 * (int(m[1]) - 1) + int(m[2]))
    return 0 if ".backbone.conv1." in name else 17 if ".compression." in name else 18


def one_flip_explains(grad, offsets, c64, c32, sd, host, target, masks, ngroups, B, bad, tries=16):
    """Is there ONE ReLU element whose fp64 input lies within FLIP_TOL of zero such that the fp64 gradient with that element's
    mask flipped meets the gradient criterion on every tensor?  Returns (call, pair, index, |x|/rms) or None."""
    near = []
    lo = max(first_relu(name) for name in bad)   # a flip at ReLU call c moves the gradients of the layers up to c only
    with torch.no_grad():
        for s in range(B):
            rl = _Relu()
            params = {k: torch.as_tensor(v).double() for k, v in sd.items() if k.rsplit(".", 1)[-1] not in ("_mean", "_var", "_count")}
            ref.forward(params, c64["buffers"], {k: torch.as_tensor(v[s:s + 1]) for k, v in host.items()}, ngroups=ngroups, train=False,
                        dtype=torch.float64, drop_masks=tuple(m[s:s + 1] for m in masks), relu=rl)
            near += [(rel, call, s, i) for rel, call, i in rl.near if call >= lo]
    for rel, call, s, i in sorted(near)[:tries]:
        base = sample_grads(sd, host, target, masks, c64["buffers"], ngroups, B, s, F.relu)
        flip = sample_grads(sd, host, target, masks, c64["buffers"], ngroups, B, s, _Relu(flip=(call, i)))
        if all(grad_ok(grad[o:o + k], c64["grads"][name] - base[name] + flip[name], c32["grads"][name])[0]
               for name, (o, k) in offsets.items()):
            return call, s, i, rel
    return None


def grad_ok(got, g64, g32):
    """The gradient criterion of test_full_resolution_gradients_against_the_fp64_checker: rel L2 <= 3 d32 + 2e-6."""
    g64 = g64.reshape(-1)
    nrm = float(g64.norm().clamp_min(1e-30))
    d32 = float((g32.reshape(-1).double() - g64).norm()) / nrm
    err = float((got - g64).norm()) / nrm
    return err <= 3.0 * d32 + 2e-6, err, d32


@pytest.fixture
def checker_threads():
    """The checker's intra-op threads for this test only (the previous setting comes back afterwards)."""
    prev = torch.get_num_threads()
    torch.set_num_threads(min(oracle.usable_cores(), 16))
    yield
    torch.set_num_threads(prev)


@pytest.mark.parametrize("B", [4, 8, 33, 34, 128, 208])
def test_training_step_matches_the_chunked_fp64_checker(B, checker_threads):
    model, sd, obs, tgt = setup(B)
    ts = VOTrainStep(model)
    out, loss = ts.forward_backward(obs, target=tgt)
    m0k, m1 = ts.dropout_masks(B)
    torch.cuda.synchronize()
    grad = ts.grad.double().cpu()
    rmv_after = {k: getattr(ts.rmv, k).detach().double().cpu().clone() for k in ("_mean", "_var", "_count")}
    ts.optimizer_step()
    torch.cuda.synchronize()
    flat = ts.flat.double().cpu()
    offsets = dict(ts.offsets)
    cfg = model.cfg
    Cc = cfg.fc_in // m0k.shape[1]                  # kernel order [B, fh*fw, 32] -> the reference's NCHW flatten [B, C*fh*fw]
    masks = (m0k[:, :, :Cc].permute(0, 2, 1).reshape(B, -1).double().cpu(), m1.double().cpu())
    host = {k: v.cpu().numpy() for k, v in obs.items()}
    target = tgt.cpu().numpy()
    del obs, ts, model
    c64 = ref.train_step_chunked(sd, host, target, ngroups=cfg.ngroups, dtype=torch.float64, drop_masks=masks)
    c32 = ref.train_step_chunked(sd, host, target, ngroups=cfg.ngroups, dtype=torch.float32, drop_masks=masks)

    l64 = float(c64["loss"])
    assert abs(loss.item() - l64) <= 1e-5 * abs(l64), (loss.item(), l64)

    rows, bad = [], []
    lr = 2.5e-4
    worst_step, off = 0.0, []
    for name, (o, k) in offsets.items():
        ok, err, d32 = grad_ok(grad[o:o + k], c64["grads"][name], c32["grads"][name])
        rows.append((name, err, d32))
        if not ok:
            bad.append((name, err, d32))
        d = (flat[o:o + k] - c64["params"][name].reshape(-1)).abs()
        worst_step = max(worst_step, float(d.max()))
        off.append((int((d > 0.1 * lr).sum()), k))
    assert set(offsets) == set(c64["grads"]) and sum(k for _, k in offsets.values()) == grad.numel()
    frac_off = sum(a for a, _ in off) / sum(k for _, k in off)
    worst = max(rows, key=lambda r: r[1] / (3 * r[2] + 2e-6))
    print(f"B={B:4d} loss {loss.item():.6g} (fp64 {l64:.6g}) | worst {worst[0]} err {worst[1]:.2e} d32 {worst[2]:.2e} | "
          f"median err {np.median([r[1] for r in rows]):.2e} median d32 {np.median([r[2] for r in rows]):.2e} | "
          f"Adam: worst {worst_step / lr:.3f} lr, {100 * frac_off:.2f} % > 0.1 lr")
    if bad:
        # the checker is ambiguous where an fp64 ReLU input lies within float32 rounding of zero: one such mask may differ
        flip = one_flip_explains(grad, offsets, c64, c32, sd, host, target, masks, cfg.ngroups, B, [n for n, _, _ in bad])
        print(f"B={B:4d} {len(bad)} tensors beyond 3 d32 + 2e-6; one near-zero mask flip of the fp64 reference "
              f"(relu call, pair, index, |x|/rms) that brings every tensor within it: {flip}")
        assert flip is not None, bad

    for k in ("_mean", "_var"):
        want = c64["buffers"][RMV + k].reshape(-1)
        got = rmv_after[k].reshape(-1)
        rel = float((got - want).norm() / want.norm())
        assert rel < 1e-5, (k, rel)
    assert float(rmv_after["_count"]) == float(c64["buffers"][RMV + "_count"])

    assert worst_step <= 2 * lr * 1.01, worst_step / lr
    assert frac_off < OFF_TOL, frac_off
