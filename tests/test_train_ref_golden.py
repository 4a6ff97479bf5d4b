"""CPU: the training-step checker (oracle/torch_train_ref.py, functional torch restatement) is pinned against golden
vectors captured from the imported reference model in train mode + the reference's own loss code + torch.optim.Adam."""
import numpy as np
import pytest
import torch

from conftest import golden_case, load_golden
from oracle import torch_train_ref as ref


def run_steps(rec, dtype, nsteps):
    cfg, sd, obs, actions = golden_case(rec)
    cur = {k: np.array(v) for k, v in sd.items()}
    state, res = None, []
    for step in range(1, nsteps + 1):
        r = ref.train_step(cur, obs, rec["target"], ngroups=cfg.ngroups, lr=float(rec["lr"]), eps=float(rec["eps"]),
                           dtype=dtype, state=state, step=step, actions=actions)
        res.append(r)
        state = r["state"]
        cur = {**{k: v.numpy() for k, v in r["params"].items()}, **{k: v.numpy() for k, v in r["buffers"].items()}}
    return res


@pytest.mark.parametrize("fname,dtype,tol", [("train_default_45x37_b4_f64.npz", torch.float64, 1e-9),
                                             ("train_act_embed_64x48_b5_f64.npz", torch.float64, 1e-9),
                                             ("train_deeper_64x48_b2_f64.npz", torch.float64, 1e-8),
                                             ("train_default_96x64_b3_f32.npz", torch.float32, 2e-3),
                                             # (appended: the ids of the cases above carry their position)
                                             ("train_wider_45x37_b3_f64.npz", torch.float64, 1e-9),
                                             ("train_rgb_dd_tdv_45x37_b3_f64.npz", torch.float64, 1e-9)])
def test_train_step_matches_reference(fname, dtype, tol):
    rec = load_golden(fname)
    steps = run_steps(rec, dtype, 2 if dtype == torch.float64 else 1)
    for s, r in enumerate(steps, start=1):
        assert abs(float(r["loss"]) - float(rec[f"loss{s}"])) <= tol * max(1.0, abs(float(rec[f"loss{s}"])))
        np.testing.assert_allclose(r["out"].double().numpy(), rec[f"out{s}"], rtol=tol, atol=tol)
        for k, g in r["grads"].items():
            gf = g.reshape(-1).double().numpy()
            nrm = float(rec[f"g{s}norm/{k}"])
            assert abs(np.linalg.norm(gf) - nrm) <= tol * max(nrm, 1e-6) * 5, k
            np.testing.assert_allclose(gf[rec[f"gidx/{k}"]], rec[f"g{s}val/{k}"], rtol=20 * tol, atol=20 * tol * max(nrm, 1e-3), err_msg=k)
            pf = r["params"][k].reshape(-1).double().numpy()
            if dtype == torch.float64:   # Adam's first step is +-lr whatever the gradient: only meaningful in fp64
                np.testing.assert_allclose(pf[rec[f"gidx/{k}"]], rec[f"p{s}val/{k}"], rtol=1e-9, atol=1e-12, err_msg=k)
        for k, b in r["buffers"].items():
            np.testing.assert_allclose(b.double().numpy().reshape(-1), rec[f"buf{s}/{k}"].reshape(-1), rtol=max(tol, 1e-6), atol=1e-7, err_msg=k)


def test_geo_inverse_loss_matches_reference():
    rec = load_golden("train_geo_loss.npz")
    d = torch.from_numpy(rec["deltas"]).requires_grad_(True)
    loss = ref.geo_inverse_loss(d, torch.from_numpy(rec["actions"]))
    loss.backward()
    assert abs(loss.item() - float(rec["loss"])) < 1e-12
    np.testing.assert_allclose(d.grad.numpy(), rec["grad"], rtol=1e-10, atol=1e-14)


@pytest.mark.parametrize("fname", ["train_joint_64x48_p4.npz", "train_joint_45x37_p3_w.npz"])
def test_joint_inverse_train_step_matches_reference_engine(fname):
    """The fp64 checker's joint iteration == the reference engine's own _process_one_batch + backward + Adam.
    Tolerances are 1e-6-ish, not 1e-10: the engine's _transfer_batch casts rgb with .float() (:335), so the reference
    divides rgb by 255 in float32 even under a float64 model; the checker divides in float64."""
    from pointnav_vo_amd import model_spec as ms, synth
    rec = load_golden(fname)
    W, H, P, seed = int(rec["width"]), int(rec["height"]), int(rec["pairs"]), int(rec["seed"])
    space = ["rgb", "depth", "discretized_depth", "top_down_view"]
    cfg = ms.config_from_kwargs(observation_space=space, observation_size=(W, H), hidden_size=512, backbone="resnet18",
                                normalize_visual_inputs=True, output_dim=3, dropout_p=0.0, discretized_depth_channels=10)
    spec = ms.state_dict_spec(cfg)
    sds = {2: synth.make_state_dict(spec, seed=seed), 3: synth.make_state_dict(spec, seed=seed + 1)}
    obs, actions, dtypes = synth.make_joint_batch(P, H, W, space, 10, seed)
    assert (actions == rec["actions"]).all() and (dtypes == rec["data_types"]).all()
    m = rec["mult"]
    r = ref.joint_train_step(sds, obs, actions, dtypes, rec["target"], ngroups=cfg.ngroups,
                             loss_inv_weight=float(rec["loss_inv_weight"]), multiplier={"dx": m[0], "dz": m[1], "dyaw": m[2]},
                             fixed=bool(rec["fixed_weights"]))
    assert abs(float(r["loss"]) - float(rec["loss"])) < 1e-7 * max(1.0, float(rec["loss"]))
    for a in (2, 3):
        idx = np.nonzero(actions == a)[0]
        np.testing.assert_allclose(r["preds"].numpy()[idx], rec[f"pred{a}"], rtol=1e-6, atol=1e-7)
        for k, g in r["grads"][a].items():
            gf = g.reshape(-1).numpy()
            nrm = float(rec[f"gnorm{a}/{k}"])
            assert abs(np.linalg.norm(gf) - nrm) <= 1e-5 * max(nrm, 1e-6), k
            np.testing.assert_allclose(gf[rec[f"gidx/{k}"]], rec[f"gval{a}/{k}"], rtol=1e-4, atol=1e-6 * max(nrm, 1e-3), err_msg=k)
            np.testing.assert_allclose(r["params"][a][k].reshape(-1).numpy()[rec[f"gidx/{k}"]], rec[f"pval{a}/{k}"],
                                       rtol=0, atol=1e-8, err_msg=k)
        for k, b in r["buffers"][a].items():
            np.testing.assert_allclose(b.numpy().reshape(-1), rec[f"buf{a}/{k}"].reshape(-1), rtol=1e-6, atol=1e-9, err_msg=k)
