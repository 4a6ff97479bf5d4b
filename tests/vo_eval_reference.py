"""numpy float64 restatement of the VO evaluation metrics (not a test module).

metrics_table restates what pnvo_vo_metrics adds for one batch (vo_cnn_engine.py:135-198 through _compute_and_update_info,
vo_cnn_regression_geo_invariance_engine.py:1259-1311); geo_inverse_diffs restates the logged values of
_compute_geo_invariance_inverse_loss (:367-449); eval_result restates the layout of eval()'s totals (:1172-1257).  Inputs are
widened to float64 first, whatever they arrive as: the float64 goldens of tests/golden/vo_eval.npz are the reference's own
arithmetic on the same float32 values.
"""
import numpy as np

EPSILON = 1e-8
DELTA_TYPES = ("dx", "dz", "dyaw")
TYPE_NAMES = {0: "cur_rel_to_prev", 1: "prev_rel_to_cur"}
MOVE_FORWARD, TURN_LEFT, TURN_RIGHT = 1, 2, 3


def slots_of(actions, data_types, acts, types):
    """model index * n_types + type index, -1 where no row takes the entry."""
    actions = np.asarray(actions).reshape(-1)
    data_types = np.asarray(data_types).reshape(-1)
    n_types = 1 if types is None else len(types)
    out = np.full(actions.shape[0], -1, np.int32)
    for e in range(actions.shape[0]):
        mi = [i for i, a in enumerate(acts) if a == -1 or a == actions[e]]
        if not mi:
            continue
        if types is None:
            out[e] = mi[0]
        elif int(data_types[e]) in list(types):
            out[e] = mi[0] * n_types + list(types).index(int(data_types[e]))
    return out


def metrics_table(pred, target, slot, n_slots, weights=None, dz_mask=None, multiplier=1.0):
    """(table [n_slots,3,4] of multiplier * {loss, abs_diff, target_magnitude, relative_diff}, count [n_slots]); a slot without
    entries stays zero."""
    pred = np.asarray(pred, np.float64).reshape(-1, 3)
    target = np.asarray(target, np.float64).reshape(-1, 3)
    slot = np.asarray(slot).reshape(-1)
    M = pred.shape[0]
    w = np.ones((M, 3)) if weights is None else np.asarray(weights, np.float64).reshape(M, 3)
    m = np.ones(M) if dz_mask is None else np.asarray(dz_mask, np.float64).reshape(M)
    table = np.zeros((n_slots, 3, 4))
    count = np.zeros(n_slots, np.int64)
    for s in range(n_slots):
        sel = np.nonzero(slot == s)[0]
        if sel.size == 0:
            continue
        count[s] = sel.size
        for d in range(3):
            sq = (target[sel, d] - pred[sel, d]) ** 2
            keep = np.arange(sel.size)
            if d == 1:
                sq = m[sel] * sq
                keep = np.nonzero(m[sel] == 1.0)[0]
            loss = np.mean(sq * w[sel, d])
            if keep.size == 0:
                abs_diff, magnitude = 0.0, EPSILON
            else:
                abs_diff = np.mean(np.sqrt(sq[keep]))
                magnitude = np.mean(np.abs(target[sel, d][keep])) + EPSILON
            table[s, d] = multiplier * np.array([loss, abs_diff, magnitude, abs_diff / magnitude])
    return table, count


def geo_inverse_diffs(deltas, actions):
    """(loss, abs_diff_rot, abs_diff_pos [2]) of alternating (cur_rel_to_prev, prev_rel_to_cur) rows, float64."""
    d = np.asarray(deltas, np.float64).reshape(-1, 3)
    a, b = d[0::2], d[1::2]
    act = np.asarray(actions).reshape(-1)[0::2]
    rot = (a[:, 2] + b[:, 2]) ** 2
    c, s = np.cos(b[:, 2]), np.sin(b[:, 2])
    pos = np.stack([b[:, 0] + c * a[:, 0] + s * a[:, 1], b[:, 1] - s * a[:, 0] + c * a[:, 1]], axis=1) ** 2
    pos[act == MOVE_FORWARD, 1] = 0.0
    return rot.mean() + pos.mean(), np.sqrt(rot).mean(), np.sqrt(pos).mean(axis=0)


def eval_result(table, count, geo, total_size, acts, types, joint):
    """The reference's layout from summed tables (each batch's multiplier = its size), geo = summed [weight * loss, rot, pos0,
    pos1] * batch size / 2."""
    n_types = 1 if types is None else len(types)
    res = {"abs_diffs": {}, "target_magnitudes": {}, "relative_diffs": {}, "counts": {}}
    for mi, act in enumerate(acts):
        for col, key in ((1, "abs_diffs"), (2, "target_magnitudes"), (3, "relative_diffs")):
            if types is None:
                res[key][act] = {d: table[mi, i, col] / total_size for i, d in enumerate(DELTA_TYPES)}
            else:
                res[key][act] = {TYPE_NAMES[t]: {d: table[mi * n_types + ti, i, col] / total_size for i, d in enumerate(DELTA_TYPES)}
                                 for ti, t in enumerate(types)}
        res["counts"][act] = (int(count[mi]) if types is None else
                              {TYPE_NAMES[t]: int(count[mi * n_types + ti]) for ti, t in enumerate(types)})
    res["objective"] = (table[:, :, 0].sum() + (2.0 * geo[0] if joint else 0.0)) / total_size
    res["abs_diff_geo_inverse_rot"] = geo[1] / (total_size / 2) if joint else None
    res["abs_diff_geo_inverse_pos"] = np.asarray(geo[2:4]) / (total_size / 2) if joint else None
    res["total_size"] = int(total_size)
    return res


def flatten_metrics(res):
    """{"abs_diffs/<act>/<type>/<d>": value, ...} of a result's three metric dicts, for comparisons."""
    out = {}
    for key in ("abs_diffs", "target_magnitudes", "relative_diffs"):
        for act, v in res[key].items():
            for k1, v1 in v.items():
                if isinstance(v1, dict):
                    for d, x in v1.items():
                        out[f"{key}/{act}/{k1}/{d}"] = float(x)
                else:
                    out[f"{key}/{act}/{k1}"] = float(v1)
    return out
