"""CPU: the host side of the VO evaluation pass (pointnav-vo_amd/evaluate.py) and the numpy restatement the GPU tests lean on.

tests/golden/vo_eval.npz holds the reference's own _process_one_batch(train_flag=False) / eval() bookkeeping on recorded
predictions (tests/golden/gen_golden_vo_eval.py); its float64 run is the reference arithmetic on the same float32 inputs."""
import inspect
import types

import numpy as np
import pytest
import torch

import vo_eval_reference as ref
from conftest import load_golden

CASES = ["a", "b", "c", "d"]
RTOL = 1e-12        # float64 on both sides, the same formulas: only the summation order inside a mean differs (~1e-16 * sqrt(n))


@pytest.fixture(scope="module")
def golden():
    return load_golden("vo_eval.npz")


def case_setup(g, case):
    acts = [int(a) for a in g[f"{case}/acts"]]
    types_ = [int(t) for t in g[f"{case}/types"]] or None
    return acts, types_, bool(int(g[f"{case}/joint"])), float(g[f"{case}/loss_inv_weight"])


def batch_tables(g, case, k, acts, types_):
    b = {n: g[f"{case}/b{k}/{n}"] for n in ("actions", "data_types", "target", "pred", "dz_mask", "weights")}
    slot = ref.slots_of(b["actions"], b["data_types"], acts, types_)
    n_slots = len(acts) * (1 if types_ is None else len(types_))
    M = b["actions"].shape[0]
    table, count = ref.metrics_table(b["pred"], b["target"], slot, n_slots, b["weights"], b["dz_mask"], multiplier=float(M))
    return b, slot, table, count


def close(a, b, rtol=RTOL):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    assert np.all(np.abs(a - b) <= rtol * np.abs(b)), (a, b)


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_float64_goldens(golden, case):
    g = golden
    acts, types_, joint, w_inv = case_setup(g, case)
    n_slots = len(acts) * (1 if types_ is None else len(types_))
    total, geo, size = np.zeros((n_slots, 3, 4)), np.zeros(4), 0
    for k in range(3):
        b, slot, table, count = batch_tables(g, case, k, acts, types_)
        M = b["actions"].shape[0]
        assert (slot >= 0).all() and (count > 0).all()
        close(table, g[f"{case}/b{k}/table_f64"])
        loss = table[:, :, 0].sum() / M
        if joint:
            valid = np.nonzero((b["actions"] == ref.TURN_LEFT) | (b["actions"] == ref.TURN_RIGHT))[0]
            gl, rot, pos = ref.geo_inverse_diffs(b["pred"][valid], b["actions"][valid])
            close(np.array([rot, pos[0], pos[1]]), g[f"{case}/b{k}/geo_f64"])
            loss += w_inv * gl
            geo += np.array([w_inv * gl, rot, pos[0], pos[1]]) * M / 2
        close(loss, g[f"{case}/b{k}/loss_f64"])
        total += table
        size += M
    assert size == int(g[f"{case}/total_size_f64"])
    close(total, g[f"{case}/total_table_f64"])
    res = ref.eval_result(total, np.zeros(n_slots, np.int64), geo, size, acts, types_, joint)
    close(res["objective"], g[f"{case}/objective_f64"])
    if joint:
        close(np.array([res["abs_diff_geo_inverse_rot"], *res["abs_diff_geo_inverse_pos"]]), g[f"{case}/geo_total_f64"])
    # the layout against the golden's own slot order: model index * n_types + type index
    tt = g[f"{case}/total_table_f64"]
    for mi, act in enumerate(acts):
        for i, d in enumerate(ref.DELTA_TYPES):
            if types_ is None:
                close(res["abs_diffs"][act][d], tt[mi, i, 1] / size)
            else:
                for ti, t in enumerate(types_):
                    close(res["relative_diffs"][act][ref.TYPE_NAMES[t]][d], tt[mi * len(types_) + ti, i, 3] / size)


def test_every_case_has_a_subset_whose_dz_mask_is_all_zero(golden):
    for case in CASES:
        tbl, M = golden[f"{case}/b0/table_f64"], golden[f"{case}/b0/actions"].shape[0]
        dead = [s for s in range(tbl.shape[0]) if tbl[s, 1, 1] == 0.0 and tbl[s, 1, 2] == 1e-8 * M and tbl[s, 1, 3] == 0.0]
        assert dead and all(tbl[s, 1, 0] == 0.0 for s in dead), case      # the masked loss of such a subset is 0 too
        assert any((golden[f"{case}/b{k}/dz_mask"] == 0).any() for k in range(3))


def test_slot_construction():
    from pointnav_vo_amd.train import regressed_types, vo_metric_slots
    F, L, R = 1, 2, 3
    actions = torch.tensor([L, R, F, F, R, L, 0, L])
    dts = torch.tensor([0, 1, 0, 1, 0, 1, 0, 2])
    assert regressed_types(()) is None
    assert regressed_types(("inverse_joint_train",)) == [0, 1] == regressed_types(("inverse_data_augment_only",))
    assert regressed_types(("something_else",)) == [0]
    # three models x two types: model index * 2 + type; the STOP entry and the entry of an unknown data type take no row
    got = vo_metric_slots(actions, dts, [F, L, R], [0, 1])
    assert got.dtype == torch.int32 and got.tolist() == [2, 5, 0, 1, 4, 3, -1, -1]
    assert got.tolist() == ref.slots_of(actions.numpy(), dts.numpy(), [F, L, R], [0, 1]).tolist()
    # only cur_rel_to_prev regressed: prev_rel_to_cur entries take no row
    assert vo_metric_slots(actions, dts, [L, R], [0]).tolist() == [0, -1, -1, -1, 1, -1, -1, -1]
    # no invariance types: one row per model, whatever the data type
    assert vo_metric_slots(actions, dts, [L, R], None).tolist() == [0, 1, -1, -1, 1, 0, -1, 0]
    # the unified model takes every entry
    assert vo_metric_slots(actions, dts, [-1], None).tolist() == [0] * 8
    assert vo_metric_slots(actions, dts, [-1], [0, 1]).tolist() == [0, 1, 0, 1, 0, 1, 0, -1]
    with pytest.raises(ValueError):
        vo_metric_slots(actions, dts, [-1, L], None)
    with pytest.raises(ValueError):
        vo_metric_slots(actions, dts, list(range(1, 10)), [0, 1])


def test_result_layout_from_a_hand_made_table():
    from pointnav_vo_amd.evaluate import layout_result
    acts, types_ = [2, 3], [0, 1]
    table = np.arange(4 * 3 * 4, dtype=np.float64).reshape(4, 3, 4) + 1.0
    count = np.array([5, 6, 7, 8])
    geo = np.array([3.0, 10.0, 20.0, 40.0])
    res = layout_result(table, count, geo, 20, acts, types_, True)
    assert set(res) == {"objective", "abs_diffs", "target_magnitudes", "relative_diffs", "abs_diff_geo_inverse_rot",
                        "abs_diff_geo_inverse_pos", "total_size", "counts"}
    # slot 3 = (act 3, prev_rel_to_cur); d = dz is row 1; columns loss, abs_diff, target_magnitude, relative_diff
    assert res["abs_diffs"][3]["prev_rel_to_cur"]["dz"] == table[3, 1, 1] / 20
    assert res["target_magnitudes"][2]["cur_rel_to_prev"]["dyaw"] == table[0, 2, 2] / 20
    assert res["relative_diffs"][2]["prev_rel_to_cur"]["dx"] == table[1, 0, 3] / 20
    assert res["counts"] == {2: {"cur_rel_to_prev": 5, "prev_rel_to_cur": 6}, 3: {"cur_rel_to_prev": 7, "prev_rel_to_cur": 8}}
    assert res["objective"] == (table[:, :, 0].sum() + 2 * 3.0) / 20
    assert res["abs_diff_geo_inverse_rot"] == 10.0 / 10 and res["abs_diff_geo_inverse_pos"].tolist() == [2.0, 4.0]
    assert res["total_size"] == 20 and isinstance(res["objective"], float)
    want = ref.eval_result(table, count, geo, 20, acts, types_, True)
    assert ref.flatten_metrics(res) == ref.flatten_metrics(want)
    # without invariance types: [act][d], no inverse-consistency values
    flat = layout_result(table[:2], count[:2], np.zeros(4), 9, [1, 2], None, False)
    assert flat["abs_diffs"][2] == {"dx": table[1, 0, 1] / 9, "dz": table[1, 1, 1] / 9, "dyaw": table[1, 2, 1] / 9}
    assert flat["counts"] == {1: 5, 2: 6} and flat["abs_diff_geo_inverse_rot"] is None and flat["abs_diff_geo_inverse_pos"] is None
    assert flat["objective"] == table[:2, :, 0].sum() / 9
    with pytest.raises(RuntimeError):
        layout_result(table, count, geo, 0, acts, types_, True)


def test_data_type_names_are_the_references():
    from pointnav_vo_amd.common_vars import DATA_TYPE_ID2STR
    assert DATA_TYPE_ID2STR == ref.TYPE_NAMES


def test_a_model_on_the_cpu_is_refused():
    from pointnav_vo_amd import vo_cnn  # noqa: F401
    from pointnav_vo_amd.evaluate import GeoInvarianceEvalStep
    from pointnav_vo_amd.registry import baseline_registry
    model = baseline_registry.get_vo_model("vo_cnn")(
        observation_space=["rgb", "depth"], observation_size=(64, 48), hidden_size=512, backbone="resnet18",
        normalize_visual_inputs=True, output_dim=3, dropout_p=0.2)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        GeoInvarianceEvalStep({2: model})
    assert model.training and model._handle is None                       # nothing was touched
    assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items())


def test_training_metrics_are_opt_in():
    from pointnav_vo_amd.train import GeoInvarianceTrainStep
    assert inspect.signature(GeoInvarianceTrainStep.__init__).parameters["metrics"].default is False
    st = GeoInvarianceTrainStep({2: types.SimpleNamespace(dev=torch.device("cpu"))})
    assert st.metrics is False and st.last_logs == {}


def test_invalid_metric_arguments_return_an_error_code_without_a_device():
    """Argument checks come before any launch, so they answer on a box without a GPU too (the pointers are never read)."""
    import ctypes as C
    from pointnav_vo_amd import _lib
    buf = np.zeros(64, np.float64)
    ptr = buf.ctypes.data_as(C.c_void_p)
    ok = [ptr, ptr, ptr, None, None, 4, 2, C.c_float(1.0), ptr, ptr]
    call = lambda a: _lib.lib.pnvo_vo_metrics(*a, None)
    for i in (0, 1, 2, 8, 9):                                             # a null required pointer
        assert call([None if j == i else v for j, v in enumerate(ok)]) == -1
    for M, n in ((0, 2), (-3, 2), (4, 0), (4, -1), (4, 17)):              # M <= 0, n_slots <= 0, n_slots above the built maximum
        assert call([M if j == 5 else n if j == 6 else v for j, v in enumerate(ok)]) == -1
        assert b"pnvo_vo_metrics" in _lib.lib.pnvo_last_error(None)
