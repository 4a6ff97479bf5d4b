"""The evaluation pass of the VO engine on the MI355X: per-action regression metrics accumulated on the device.

Mirrors VOCNNRegressionGeometricInvarianceEngine.eval (pointnav_vo/vo/engine/vo_cnn_regression_geo_invariance_engine.py:
1020-1257) around _process_one_batch(train_flag=False) (:451-807): every action model, in eval(), sees the entries of its
action; per action model, per regressed data type and per delta component the engine adds up abs_diff, target_magnitude,
relative_diff and the objective, each times the batch size (_compute_and_update_info :1259-1311 around vo_cnn_engine.py:135-198,
update="sum"); with "inverse_joint_train" the two inverse-consistency diffs of the predictions in batch order are added up
times half the batch size (:1123-1129).  Checkpoint selection and every VO number of the paper come from these totals.

Here the forwards are the models' eval kernels, the table of a batch is ONE launch (pnvo_vo_metrics, float64, a fixed summation
order) that adds into totals living on the device, and the inverse-consistency diffs are pnvo_geo_inverse_loss without a
gradient.  Index bookkeeping stays on the host as in the reference and in train.GeoInvarianceTrainStep; what it produces reaches
the device through pinned memory, so `step` never waits for the device — a pass is enqueued batch after batch and `result()`
synchronises once.  (The first forward after a model's weights changed uploads them, as every eval forward of this package does.)

Single process only: the reference's eval has no distributed branch, and neither has this.

Departure from the reference: an (action model, data type) subset WITHOUT entries in a batch adds nothing, and a batch without
turn entries adds nothing to the inverse-consistency totals, where the reference takes the mean of an empty tensor and carries
NaN through its totals.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .common_vars import DATA_TYPE_ID2STR, DEFAULT_DELTA_TYPES
from .train import (CUR_REL_TO_PREV, MOVE_FORWARD, PREV_REL_TO_CUR, TURN_LEFT, TURN_RIGHT, _ptr, compute_loss_weights,
                    launch_vo_metrics, regressed_types, to_device_async, vo_metric_slots)


def layout_result(table, count, geo, total_size, acts, types, joint):
    """The reference's layout of an evaluation's totals (engine :1172-1257) from the host copies of the device totals: table
    [n_slots,3,4] of summed {loss, abs_diff, target_magnitude, relative_diff} * batch size, count [n_slots], geo [4] of summed
    pnvo_geo_inverse_loss outputs * batch size / 2.  Metric dicts are [act][data type name][d] (or [act][d] when `types` is None)
    and hold total / total_size; the inverse-consistency diffs hold total / (total_size / 2), None unless `joint`."""
    table = np.asarray(table, dtype=np.float64)
    count = np.asarray(count, dtype=np.int64)
    geo = np.asarray(geo, dtype=np.float64)
    n_types = 1 if types is None else len(types)
    assert table.shape == (len(acts) * n_types, 3, 4) and count.shape == (len(acts) * n_types,)
    if total_size <= 0:
        raise RuntimeError("the evaluation has seen no batch")
    res = {"abs_diffs": {}, "target_magnitudes": {}, "relative_diffs": {}, "counts": {}}
    for mi, act in enumerate(acts):
        for col, key in ((1, "abs_diffs"), (2, "target_magnitudes"), (3, "relative_diffs")):
            if types is None:
                res[key][act] = {d: float(table[mi, i, col] / total_size) for i, d in enumerate(DEFAULT_DELTA_TYPES)}
            else:
                res[key][act] = {DATA_TYPE_ID2STR[t]: {d: float(table[mi * n_types + ti, i, col] / total_size)
                                                       for i, d in enumerate(DEFAULT_DELTA_TYPES)} for ti, t in enumerate(types)}
        res["counts"][act] = (int(count[mi]) if types is None else
                              {DATA_TYPE_ID2STR[t]: int(count[mi * n_types + ti]) for ti, t in enumerate(types)})
    # the objective: every regression loss and loss_inv_weight * the inverse loss, each times its batch's size (:1110-1111);
    # geo[0] was summed times batch size / 2 like the diffs beside it
    res["objective"] = float((table[:, :, 0].sum() + (2.0 * geo[0] if joint else 0.0)) / total_size)
    res["abs_diff_geo_inverse_rot"] = float(geo[1] / (total_size / 2)) if joint else None
    res["abs_diff_geo_inverse_pos"] = geo[2:4] / (total_size / 2) if joint else None
    res["total_size"] = int(total_size)
    return res


class GeoInvarianceEvalStep:
    """eval() of VOCNNRegressionGeometricInvarianceEngine for a dict of action models: `step` per batch, `result()` at the end.

    models: {act: model} with act in {-1 (all actions), MOVE_FORWARD, TURN_LEFT, TURN_RIGHT}, registered VO models on the
    device; act-embed models are handed the entries' actions.  loss_weight_fixed / loss_weight_multiplier: VO.TRAIN's, for
    train.compute_loss_weights.  Single process only (the reference's eval has no distributed branch)."""

    def __init__(self, models, invariance_types=("inverse_joint_train",), loss_inv_weight=1.0, loss_weight_fixed=True,
                 loss_weight_multiplier=None, save_pred=False):
        self.models = dict(models)
        if not self.models:
            raise ValueError("GeoInvarianceEvalStep needs at least one action model")
        self.invariance_types = tuple(invariance_types)
        self.loss_inv_weight = float(loss_inv_weight)
        self.loss_weight_fixed = bool(loss_weight_fixed)
        self.loss_weight_multiplier = dict(loss_weight_multiplier) if loss_weight_multiplier else None
        self.save_pred = bool(save_pred)
        self.dev = self._check_devices()
        self.acts = list(self.models.keys())
        self.types = regressed_types(self.invariance_types)
        self.joint = "inverse_joint_train" in self.invariance_types
        self.n_slots = len(self.acts) * (1 if self.types is None else len(self.types))
        vo_metric_slots(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), self.acts, self.types)   # validates
        # unit weights are passed as "no weights"
        self._unit_weights = self.loss_weight_fixed and all(
            float(v) == 1.0 for v in (self.loss_weight_multiplier or {"dx": 1.0}).values())
        self._table = torch.zeros((self.n_slots, 3, 4), device=self.dev, dtype=torch.float64)
        self._count = torch.zeros(self.n_slots, device=self.dev, dtype=torch.int64)
        self._geo = torch.zeros(4, device=self.dev, dtype=torch.float64)
        self.reset()

    def _check_devices(self):
        devs = {next(m.parameters()).device for m in self.models.values()}
        if any(d.type != "cuda" for d in devs):
            raise RuntimeError("GeoInvarianceEvalStep runs on an MI355X only: move the models with .to('cuda') first "
                               "(there is no CPU fallback)")
        if len(devs) != 1:
            raise RuntimeError(f"the action models are on different devices: {sorted(map(str, devs))}")
        return next(iter(devs))

    def reset(self):
        """Clear the totals (asynchronous)."""
        self._table.zero_()
        self._count.zero_()
        self._geo.zero_()
        self.total_size = 0
        self._saved = []                      # per step: (gt rows, pred rows) on the device, host index lists per subset

    def step(self, batch, actions, data_types, targets, dz_regress_masks=None, chunk_idxs=None, entry_idxs=None):
        """batch: dict of NHWC device tensors [M,...] (the models' observation_pairs); actions [M] int and data_types [M]
        (CUR_REL_TO_PREV / PREV_REL_TO_CUR), host tensors as the dataloader hands them; targets [M,3] (dx, dz, dyaw);
        dz_regress_masks [M]; chunk_idxs / entry_idxs [M] (needed with save_pred).  Returns the predictions [M,3] in batch order
        (device, rows of entries no model takes are 0).  Never waits for the device as long as the host-side arguments are host
        tensors (non-fixed loss weights are a host function of the targets)."""
        dev = self._check_devices()
        actions = torch.as_tensor(actions).reshape(-1).to("cpu", torch.int64)
        data_types = torch.as_tensor(data_types).reshape(-1).to("cpu", torch.int64)
        M = actions.numel()
        if M == 0:
            raise ValueError("an evaluation batch needs at least one entry")
        targets = torch.as_tensor(targets, dtype=torch.float32).reshape(-1, 3)
        if targets.shape[0] != M or data_types.numel() != M:
            raise ValueError(f"{M} actions, {data_types.numel()} data types, {targets.shape[0]} targets")
        if self.save_pred and (chunk_idxs is None or entry_idxs is None):
            raise ValueError("save_pred needs chunk_idxs and entry_idxs")
        weights = None
        if not self._unit_weights:
            lw = compute_loss_weights(actions, targets if not self.loss_weight_fixed else torch.zeros(M, 3),
                                      multiplier=self.loss_weight_multiplier, fixed=self.loss_weight_fixed)
            weights = to_device_async(torch.stack([lw[k] for k in DEFAULT_DELTA_TYPES], dim=1), dev)
        tdev = to_device_async(targets, dev).contiguous()
        mask = None
        if dz_regress_masks is not None:
            mask = to_device_async(torch.as_tensor(dz_regress_masks, dtype=torch.float32).reshape(-1), dev).contiguous()
            assert mask.numel() == M
        slot = to_device_async(vo_metric_slots(actions, data_types, self.acts, self.types), dev)
        a_dev = None
        if any(m.cfg.act_embed for m in self.models.values()):
            a_dev = to_device_async(actions, dev)
        preds = torch.zeros((M, 3), device=dev, dtype=torch.float32)
        for model in self.models.values():
            model.eval()
        subsets = {}
        with torch.cuda.device(dev), torch.no_grad():
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            for act, model in self.models.items():
                idx = torch.arange(M) if act == -1 else torch.nonzero(actions == act, as_tuple=True)[0]
                if idx.numel() == 0:
                    continue
                subsets[act] = idx
                if act == -1:
                    preds = model(batch, a_dev if model.cfg.act_embed else None)
                    continue
                di = to_device_async(idx, dev)
                sub = {k: v.index_select(0, di) for k, v in batch.items()}
                out = model(sub, a_dev.index_select(0, di) if model.cfg.act_embed else None)
                preds.index_copy_(0, di, out)
            launch_vo_metrics(preds, tdev, slot, weights, mask, self.n_slots, float(M), self._table, self._count, stream)
            if self.joint:
                valid = torch.nonzero((actions == TURN_LEFT) | (actions == TURN_RIGHT), as_tuple=True)[0]
                if valid.numel():
                    vt = data_types[valid]
                    if valid.numel() % 2 or not bool((vt[0::2] == CUR_REL_TO_PREV).all() and (vt[1::2] == PREV_REL_TO_CUR).all()):
                        raise AssertionError("inverse_joint_train expects alternating (cur_rel_to_prev, prev_rel_to_cur) entries")
                    d = preds.index_select(0, to_device_async(valid, dev)).contiguous()
                    a32 = to_device_async(actions[valid].to(torch.int32), dev)
                    out4 = torch.empty(4, device=dev)
                    _lib.check(_lib.lib.pnvo_geo_inverse_loss(_ptr(d), _ptr(a32), int(d.shape[0]), MOVE_FORWARD,
                                                              C.c_float(self.loss_inv_weight), _ptr(out4), None, stream))
                    self._geo.add_(out4.double(), alpha=M / 2)
            if self.save_pred:
                ids = torch.stack([torch.as_tensor(chunk_idxs).reshape(-1).to("cpu", torch.float64),
                                   torch.as_tensor(entry_idxs).reshape(-1).to("cpu", torch.float64)], dim=1)
                ids = to_device_async(ids, dev)
                self._saved.append((torch.cat((ids, tdev.double()), dim=1), torch.cat((ids, preds.double()), dim=1),
                                    {act: (idx.numpy(), data_types[idx].numpy()) for act, idx in subsets.items()}))
        self.total_size += M
        return preds

    def _saved_rows(self):
        """gt / pred rows [chunk_idx, entry_idx, dx, dz, dyaw] per action (and per regressed data type), as :624-729 keeps them."""
        gt, pred = {}, {}
        for g_dev, p_dev, subsets in self._saved:
            g, p = g_dev.cpu().numpy(), p_dev.cpu().numpy()
            for act, (idx, dt) in subsets.items():
                if self.types is None:
                    gt.setdefault(act, []).append(g[idx])
                    pred.setdefault(act, []).append(p[idx])
                    continue
                for t in self.types:
                    sel = idx[dt == t]
                    gt.setdefault(act, {}).setdefault(t, []).append(g[sel])
                    pred.setdefault(act, {}).setdefault(t, []).append(p[sel])
        cat = lambda v: {t: np.concatenate(r, axis=0) for t, r in v.items()} if isinstance(v, dict) else np.concatenate(v, axis=0)
        return {a: cat(v) for a, v in gt.items()}, {a: cat(v) for a, v in pred.items()}

    def result(self):
        """One synchronisation, then plain Python / numpy values in the reference's layout: {"objective", "abs_diffs",
        "target_magnitudes", "relative_diffs", "abs_diff_geo_inverse_rot", "abs_diff_geo_inverse_pos", "total_size", "counts"}
        (+ "gt", "pred" with save_pred) — see layout_result."""
        torch.cuda.current_stream(self.dev).synchronize()
        res = layout_result(self._table.cpu().numpy(), self._count.cpu().numpy(), self._geo.cpu().numpy(), self.total_size,
                            self.acts, self.types, self.joint)
        if self.save_pred:
            res["gt"], res["pred"] = self._saved_rows()
        return res
