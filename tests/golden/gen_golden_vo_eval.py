#!/usr/bin/env python
"""Generate tests/golden/vo_eval.npz: the metric arithmetic of the reference's evaluation pass (build container only, CPU).

    python tests/golden/gen_golden_vo_eval.py

The reference's own _process_one_batch(..., train_flag=False) (vo_cnn_regression_geo_invariance_engine.py:451-807) runs over three
batches per case (the last one short) with the defaultdict totals of eval() (:1043-1063), on an engine built the way
gen_golden.py builds the one of the training goldens (object.__new__ + a namespace config).  The action models are STUBS that
return recorded predictions — the fixture pins the metric arithmetic, independent of any network; an observation tensor of one
column carries each entry's row number to them.  Every case runs twice on the same float32 values: once on float32 tensors (the
reference as it runs) and once on float64 tensors with float64 as torch's default dtype (the constants the reference creates —
torch.zeros(1) + EPSILON, the masks — are then float64 too).  The loss weights of the float64 run are the float32 run's widened:
they are an input of the metrics, like the predictions and the targets.  The only addition to the engine is a subclass method
that records the return value of _compute_and_update_info (the per-subset loss, which eval() only keeps summed).

Stored per case X in (a, b, c, d): the configuration; per batch k the inputs (actions, data_types, target, pred, dz_mask,
weights) and, per run R in (f32, f64), the batch's table [n_slots,3,4] of {loss, abs_diff, target_magnitude, relative_diff} *
cur_batch_size from FRESH totals (slot = model index * n_types + type index), its total loss and its inverse-consistency diffs;
and the accumulated totals of a pass over the three batches with eval()'s bookkeeping: total table, objective, the diffs over
total_size / 2, total_size.  The fixtures are data: no reference source text is stored.
"""
import importlib
import os
import sys
from collections import defaultdict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as gg  # noqa: E402

D_TYPES = ["dx", "dz", "dyaw"]
MOVE_FORWARD, TURN_LEFT, TURN_RIGHT = 1, 2, 3

CASES = {
    # acts of the models, invariance types, loss_weight_fixed, multiplier, samples per batch
    "a": dict(acts=[MOVE_FORWARD, TURN_LEFT, TURN_RIGHT], inv=["inverse_joint_train"], fixed=True,
              mult={"dx": 1.0, "dz": 2.0, "dyaw": 0.5}, samples=[7, 7, 3]),
    "b": dict(acts=[MOVE_FORWARD, TURN_LEFT, TURN_RIGHT], inv=["inverse_joint_train"], fixed=False,
              mult={"dx": 2.0, "dz": 1.5, "dyaw": 3.0}, samples=[8, 6, 3]),
    "c": dict(acts=[-1], inv=[], fixed=True, mult={"dx": 1.0, "dz": 1.0, "dyaw": 1.0}, samples=[13, 11, 5]),
    "d": dict(acts=[TURN_LEFT, TURN_RIGHT], inv=["inverse_data_augment_only"], fixed=True,
              mult={"dx": 1.0, "dz": 1.0, "dyaw": 1.0}, samples=[6, 7, 2]),
}
LOSS_INV_WEIGHT = 0.7


class StubModel:
    """An action model that returns recorded predictions: row numbers arrive in the one column of the "depth" observation."""

    def __init__(self):
        self.table = None

    def eval(self):
        return self

    def __call__(self, batch_pairs, actions=None):
        return self.table[batch_pairs["depth"][:, 0].long()]


def make_batch(case, spec, k, cv):
    """Inputs of batch k: float32 values, every (action model, data type) subset non-empty, a dz mask with zeros and one subset
    whose mask is all zero."""
    rng = np.random.RandomState(1000 * (ord(case) - ord("a") + 1) + k)
    n = spec["samples"][k]
    paired = len(spec["inv"]) > 0                    # the dataset adds each sample's prev_rel_to_cur entry (swapped turn)
    pool = [a for a in (MOVE_FORWARD, TURN_LEFT, TURN_RIGHT) if -1 in spec["acts"] or a in spec["acts"]]
    acts = np.array(pool + list(rng.choice(pool, n - len(pool))) if n >= len(pool) else pool[:n], dtype=np.int64)
    rng.shuffle(acts)
    if paired:
        opp = {MOVE_FORWARD: MOVE_FORWARD, TURN_LEFT: TURN_RIGHT, TURN_RIGHT: TURN_LEFT}
        actions = np.array([x for a in acts for x in (a, opp[int(a)])], dtype=np.int64)
        dtypes = np.tile(np.array([cv.CUR_REL_TO_PREV, cv.PREV_REL_TO_CUR], dtype=np.int64), n)
    else:
        actions, dtypes = acts, np.full(n, cv.CUR_REL_TO_PREV, dtype=np.int64)
    M = actions.shape[0]
    clean = np.array([cv.NO_NOISE_DELTAS[int(a)] for a in actions])
    target = (clean + 1e-2 * rng.standard_normal((M, 3))).astype(np.float32)
    pred = (target + 3e-2 * rng.standard_normal((M, 3))).astype(np.float32)
    mask = (rng.uniform(size=M) < 0.7).astype(np.float32)
    mask[0] = 0.0
    # One subset without a mask == 1 entry, in the FIRST batch: the reference returns a [1]-shaped tensor for such a subset and a
    # 0-dim one otherwise, and its `total += value` cannot add the former into a total that already holds the latter (:1303).
    dead = np.ones(M, bool) if -1 in spec["acts"] else (actions == spec["acts"][-1]) & (dtypes == cv.CUR_REL_TO_PREV)
    for act in spec["acts"]:
        for t in sorted(set(dtypes.tolist())):
            sel = (np.ones(M, bool) if act == -1 else actions == act) & (dtypes == t)
            if k == 0 and (sel & dead).any():
                mask[sel] = 0.0
            elif not mask[sel].any():
                mask[np.nonzero(sel)[0][-1]] = 1.0
    return dict(actions=actions, data_types=dtypes, target=target, pred=pred, dz_mask=mask)


def build_engine(Engine, spec, weights_from=None):
    class Recording(Engine):
        def _compute_and_update_info(self, act, d_type, *a, **kw):
            loss = Engine._compute_and_update_info(self, act, d_type, *a, **kw)
            self.recorded_losses[(act, kw.get("data_type_name"), d_type)] = float(loss)
            return loss

        def _compute_loss_weights(self, actions, dxs, dys, dyaws):
            w = Engine._compute_loss_weights(self, actions, dxs.float(), dys.float(), dyaws.float())
            self.recorded_weights = {k: v.detach().clone() for k, v in w.items()}
            return {k: v.to(dxs.dtype) for k, v in w.items()}

    eng = object.__new__(Recording)
    eng._config = gg._NS(VO=gg._NS(GEOMETRY=gg._NS(loss_inv_weight=LOSS_INV_WEIGHT, invariance_types=list(spec["inv"])),
                                   TRAIN=gg._NS(loss_weight_fixed=spec["fixed"], loss_weight_multiplier=dict(spec["mult"])),
                                   MODEL=gg._NS(name="vo_cnn")))
    eng._verbose = False
    eng.device = torch.device("cpu")
    eng._pin_memory_flag = False
    eng._data_collate_mode = "normal"
    eng._observation_space = ["depth"]
    eng._act_type = -1 if spec["acts"] == [-1] else list(spec["acts"])
    if isinstance(eng._act_type, list) and MOVE_FORWARD in eng._act_type:
        eng._act_type = "separate"                   # (a list means "turn actions only" to the engine's sanity check, :540-543)
    eng._act_list = list(spec["acts"])
    eng.vo_model = {a: StubModel() for a in spec["acts"]}
    eng.recorded_losses = {}
    return eng


def batch_data(b, dtype):
    t = lambda a, dt=dtype: torch.from_numpy(np.ascontiguousarray(a)).to(dt)
    M = b["actions"].shape[0]
    tg = t(b["target"])
    rows = torch.arange(M).to(dtype).unsqueeze(1)
    none = torch.zeros(M, 1)
    return (t(b["data_types"], torch.int64).unsqueeze(1), none, rows, none, none, t(b["actions"], torch.int64).unsqueeze(1),
            tg[:, 0:1], torch.zeros_like(tg[:, 0:1]), tg[:, 1:2], tg[:, 2:3], t(b["dz_mask"]).unsqueeze(1),
            torch.zeros(M, 1, dtype=torch.int64), torch.arange(M).unsqueeze(1))


def fresh_totals(spec):
    mk = (lambda: defaultdict(float)) if len(spec["inv"]) == 0 else (lambda: defaultdict(lambda: defaultdict(float)))
    return tuple({a: mk() for a in spec["acts"]} for _ in range(3))


def slot_names(spec, cv):
    if len(spec["inv"]) == 0:
        return [(a, None) for a in spec["acts"]], None
    types = [cv.CUR_REL_TO_PREV, cv.PREV_REL_TO_CUR]        # every case with invariance types regresses both (:682-687)
    return [(a, cv.DATA_TYPE_ID2STR[t]) for a in spec["acts"] for t in types], types


def table_of(totals, losses, slots, scale):
    """[n_slots,3,4]: column 0 from the recorded per-subset losses * scale, columns 1-3 from the engine's totals."""
    out = np.zeros((len(slots), 3, 4))
    for s, (act, name) in enumerate(slots):
        for i, d in enumerate(D_TYPES):
            node = [tot[act] if name is None else tot[act][name] for tot in totals]
            out[s, i, 0] = losses[(act, name, d)] * scale
            out[s, i, 1:] = [float(x[d]) for x in node]
    return out


def run_case(Engine, case, spec, cv, dtype, batches):
    """One run of the reference over the case's batches at `dtype`: per-batch records from fresh totals, then eval()'s pass."""
    torch.set_default_dtype(dtype)
    try:
        slots, _ = slot_names(spec, cv)
        joint = "inverse_joint_train" in spec["inv"]
        eng = build_engine(Engine, spec)
        rec = {}

        def one(b, totals):
            for m in eng.vo_model.values():
                m.table = torch.from_numpy(b["pred"]).to(dtype)
            with torch.no_grad():
                return eng._process_one_batch(batch_data(b, dtype), list(spec["inv"]), *totals, train_flag=False)

        for k, b in enumerate(batches):
            totals = fresh_totals(spec)
            loss, bs, _, _, infos = one(b, totals)
            assert bs == b["actions"].shape[0]
            for (act, name) in slots:                # the reference itself must produce no NaN: no empty subset
                sel = (np.ones(bs, bool) if act == -1 else b["actions"] == act)
                if name is not None:
                    sel = sel & (b["data_types"] == {v: k_ for k_, v in cv.DATA_TYPE_ID2STR.items()}[name])
                assert sel.any(), (case, k, act, name)
            rec[f"b{k}/table"] = table_of(totals, eng.recorded_losses, slots, bs)
            rec[f"b{k}/loss"] = float(loss)
            rec[f"b{k}/weights"] = torch.cat([eng.recorded_weights[d] for d in D_TYPES], dim=1).numpy()
            if joint:
                rec[f"b{k}/geo"] = np.array([float(infos[3])] + [float(x) for x in infos[4]])
            assert np.isfinite(rec[f"b{k}/table"]).all() and np.isfinite(rec[f"b{k}/loss"])
        # eval() :1043-1129, :1190-1215
        totals = fresh_totals(spec)
        total_size, total_loss, geo_rot, geo_pos = 0, 0.0, 0.0, 0.0
        loss_table = np.zeros((len(slots), 3))
        for b in batches:
            loss, bs, _, _, infos = one(b, totals)
            total_size += bs
            total_loss += loss * bs
            for s, (act, name) in enumerate(slots):
                for i, d in enumerate(D_TYPES):
                    loss_table[s, i] += eng.recorded_losses[(act, name, d)] * bs
            if joint:
                geo_rot += infos[3] * bs / 2
                geo_pos += infos[4] * bs / 2
        tt = table_of(totals, defaultdict(float), slots, 0.0)
        tt[:, :, 0] = loss_table
        rec["total_table"] = tt
        rec["objective"] = float(total_loss) / total_size
        rec["total_size"] = total_size
        if joint:
            rec["geo_total"] = np.array([float(geo_rot / (total_size / 2))] + [float(x) for x in geo_pos / (total_size / 2)])
        return rec
    finally:
        torch.set_default_dtype(torch.float32)


def main():
    gg.import_reference()
    Engine = gg.import_geo_engine()
    cv = importlib.import_module("pointnav_vo.vo.common.common_vars")
    out = {}
    for case, spec in CASES.items():
        batches = [make_batch(case, spec, k, cv) for k in range(3)]
        assert any((b["dz_mask"] == 0).any() for b in batches)
        runs = {tag: run_case(Engine, case, spec, cv, dt, batches) for tag, dt in (("f32", torch.float32), ("f64", torch.float64))}
        slots, types = slot_names(spec, cv)
        out[f"{case}/acts"] = np.array(spec["acts"], dtype=np.int64)
        out[f"{case}/types"] = np.array(types if types is not None else [], dtype=np.int64)
        out[f"{case}/joint"] = np.array(int("inverse_joint_train" in spec["inv"]))
        out[f"{case}/invariance_types"] = np.array(",".join(spec["inv"]))
        out[f"{case}/fixed"] = np.array(int(spec["fixed"]))
        out[f"{case}/mult"] = np.array([spec["mult"][d] for d in D_TYPES])
        out[f"{case}/loss_inv_weight"] = np.array(LOSS_INV_WEIGHT)
        for k, b in enumerate(batches):
            for name, v in b.items():
                out[f"{case}/b{k}/{name}"] = v
            assert np.array_equal(runs["f32"][f"b{k}/weights"], runs["f64"][f"b{k}/weights"])
            out[f"{case}/b{k}/weights"] = runs["f32"][f"b{k}/weights"].astype(np.float32)
        for tag, rec in runs.items():
            for name, v in rec.items():
                if name.endswith("/weights"):
                    continue
                out[f"{case}/{name}_{tag}"] = np.asarray(v)
        # both runs took the same subsets and branches (not a precision statement)
        for name, v in runs["f64"].items():
            a, b = np.asarray(runs["f32"][name], np.float64), np.asarray(v, np.float64)
            assert np.all(np.abs(a - b) <= 1e-4 * np.abs(b)), (case, name, a, b)
        dead = [k for k in range(3) if (runs["f64"][f"b{k}/table"][:, 1, 1:] == np.array([0.0, 1e-8 * batches[k]["actions"].shape[0], 0.0])).all(axis=1).any()]
        assert dead, f"case {case}: no subset with an all-zero dz mask"
        print(f"case {case}: objective {runs['f64']['objective']:.8f} (float32 run {runs['f32']['objective']:.8f}), "
              f"total_size {runs['f64']['total_size']}, all-zero-mask subset in batch {dead}")
    path = os.path.join(HERE, "vo_eval.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 100 * 1024


if __name__ == "__main__":
    main()
