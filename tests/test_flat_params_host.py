"""flat_params.FlatParams on CPU tensors: the layout, the aliasing, the change signature and the Adam state round trip that VOTrainStep
and PolicyTrainStep both build on.  No library call is made (adam_step is the only method that needs one)."""
import pytest
import torch
import torch.nn as nn

from pointnav_vo_amd import ppo
from pointnav_vo_amd.flat_params import FlatParams

SIZES = {"a": (3,), "b": (5, 1), "h.c": (2, 4), "h.d": (1,)}          # 3, 5, 8 and 1 floats: align=4 leaves gaps after a, b and h.d
TAIL = 6


class _Holder(nn.Module):
    pass


def make_module(seed=0):
    g = torch.Generator().manual_seed(seed)
    m = _Holder()
    m.a = nn.Parameter(torch.randn(3, generator=g))
    m.b = nn.Parameter(torch.randn(5, 1, generator=g))
    m.h = _Holder()
    m.h.c = nn.Parameter(torch.randn(2, 4, generator=g))
    m.h.d = nn.Parameter(torch.randn(1, generator=g))
    return m


def make_store(align, tail=0, seed=0):
    m = make_module(seed)
    named = list(m.named_parameters())
    assert [(n, tuple(p.shape)) for n, p in named] == list(SIZES.items())
    values = {n: p.detach().clone() for n, p in named}
    return m, FlatParams(named, torch.device("cpu"), align=align, tail=tail), values


def test_tight_layout_is_the_running_sum_of_numel():
    _, st, _ = make_store(1)
    assert st.offsets == {"a": (0, 3), "b": (3, 5), "h.c": (8, 8), "h.d": (16, 1)}
    assert st.n_params == 17
    assert st.flat.numel() == st.grad.numel() == st.exp_avg.numel() == st.exp_avg_sq.numel() == 17


def test_aligned_layout_is_ppo_flat_offsets():
    _, st, _ = make_store(4, TAIL)
    offsets, used = ppo.flat_offsets(list(SIZES.items()))
    assert st.offsets == offsets == {"a": (0, 3), "b": (4, 5), "h.c": (12, 8), "h.d": (20, 1)}
    assert st.n_params == used == 24
    assert st.flat.numel() == st.grad.numel() == 24 + TAIL and st.exp_avg.numel() == st.exp_avg_sq.numel() == 24


@pytest.mark.parametrize("align,tail", [(1, 0), (4, TAIL)])
def test_parameters_alias_the_buffers_and_the_rest_is_zero(align, tail):
    m, st, values = make_store(align, tail)
    covered = torch.zeros(st.flat.numel(), dtype=torch.bool)
    for n, p in m.named_parameters():
        off, k = st.offsets[n]
        assert p.data_ptr() == st.flat.data_ptr() + 4 * off and p.grad.data_ptr() == st.grad.data_ptr() + 4 * off
        assert p.shape == values[n].shape == p.grad.shape
        assert torch.equal(st.flat[off:off + k], values[n].reshape(-1))
        covered[off:off + k] = True
    assert int((~covered).sum()) == st.flat.numel() - 17
    assert not st.flat[~covered].any() and not st.grad.any() and not st.exp_avg.any() and not st.exp_avg_sq.any()
    assert not st.changed()


def test_in_place_edit_is_seen_and_already_in_the_buffer():
    """An in-place edit needs no realias(): the parameter IS the flat buffer.  changed() reads torch's version counter, which counts
    in-place writes to the parameter (load_state_dict's p.copy_, an edit under no_grad).  A write through `p.data` (p.data.add_(1)) goes
    through a detached alias with a version counter of its own (torch: p._version stays), so it lands in the flat buffer all the same
    but no signature of (data_ptr, _version) can see it; the parent's train steps had the same blind spot."""
    m, st, values = make_store(4, TAIL)
    off, k = st.offsets["h.c"]
    m.h.c.data.add_(1)
    assert torch.equal(st.flat[off:off + k], (values["h.c"] + 1).reshape(-1))
    with torch.no_grad():
        m.h.c.add_(1)
    assert st.changed()
    assert torch.equal(st.flat[off:off + k], (values["h.c"] + 2).reshape(-1))
    assert m.h.c.data_ptr() == st.flat.data_ptr() + 4 * off
    st.mark()
    assert not st.changed()
    m.load_state_dict({n: v for n, v in values.items()})                           # what a resume does
    assert st.changed() and torch.equal(st.flat[off:off + k], values["h.c"].reshape(-1))


def test_repointed_parameter_is_copied_in_and_aliased_again():
    m, st, values = make_store(4, TAIL)
    other = torch.full((5, 1), 7.0)
    m.b.data = other
    assert st.changed()
    off, k = st.offsets["b"]
    assert torch.equal(st.flat[off:off + k], values["b"].reshape(-1))         # not yet
    st.realias()
    assert torch.equal(st.flat[off:off + k], other.reshape(-1))
    assert m.b.data_ptr() == st.flat.data_ptr() + 4 * off and m.b.grad.data_ptr() == st.grad.data_ptr() + 4 * off
    for n in ("a", "h.c", "h.d"):                                                   # the others were left alone
        o, kk = st.offsets[n]
        assert torch.equal(st.flat[o:o + kk], values[n].reshape(-1))
    assert not st.flat[9:12].any() and not st.flat[24:].any()
    st.mark()
    assert not st.changed()


def test_adam_state_round_trip_over_a_subset_of_names():
    _, st, _ = make_store(4, TAIL)
    g = torch.Generator().manual_seed(1)
    st.exp_avg.copy_(torch.randn(24, generator=g))
    st.exp_avg_sq.copy_(torch.rand(24, generator=g))
    m0, v0 = st.exp_avg.clone(), st.exp_avg_sq.clone()
    names = ["a", "h.c"]
    sd = st.adam_state_dict(names, 5, 1e-3, (0.9, 0.99), 1e-6)
    assert list(sd["state"]) == [0, 1] and sd["param_groups"][0]["params"] == [0, 1]
    assert sd["state"][1]["exp_avg"].shape == (2, 4) and float(sd["state"][0]["step"]) == 5.0
    st.exp_avg[0:3] = -1.0                                                      # a and c are overwritten by the load ...
    st.exp_avg_sq[12:20] = -1.0
    st.exp_avg[4:9] = 3.0                                                       # ... b, outside `names`, stays as it is now
    m0[4:9] = 3.0
    step, group = st.load_adam_state_dict(sd, names)
    assert step == 5 and group["lr"] == 1e-3 and tuple(group["betas"]) == (0.9, 0.99) and group["eps"] == 1e-6
    assert torch.equal(st.exp_avg, m0) and torch.equal(st.exp_avg_sq, v0)
    del sd["state"][1]                                                          # a parameter without state: zero moments
    assert st.load_adam_state_dict(sd, names)[0] == 5
    assert not st.exp_avg[12:20].any() and not st.exp_avg_sq[12:20].any() and torch.equal(st.exp_avg[:12], m0[:12])


def test_differing_step_counts_raise():
    _, st, _ = make_store(1)
    names = list(SIZES)
    sd = st.adam_state_dict(names, 3, 1e-3, (0.9, 0.999), 1e-8)
    sd["state"][2]["step"] = torch.tensor(4.0)
    with pytest.raises(ValueError, match="step counts differ"):
        st.load_adam_state_dict(sd, names)


def test_state_dict_has_torch_adams_layout():
    m, st, _ = make_store(1)
    names = list(SIZES)
    sd = st.adam_state_dict(names, 2, 1e-3, (0.9, 0.999), 1e-8)
    opt = torch.optim.Adam(list(m.parameters()), lr=0.5)
    opt.load_state_dict(sd)
    assert opt.param_groups[0]["lr"] == 1e-3
    for n, p in m.named_parameters():
        off, k = st.offsets[n]
        assert torch.equal(opt.state[p]["exp_avg"].reshape(-1), st.exp_avg[off:off + k]) and float(opt.state[p]["step"]) == 2.0
    assert set(opt.state_dict()["param_groups"][0]) >= set(sd["param_groups"][0])
