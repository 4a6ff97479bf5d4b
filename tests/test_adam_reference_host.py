"""CPU: tests/adam_reference.py's trajectory (the real torch.optim.Adam, fresh and resumed through load_state_dict) pins
oracle.torch_train_ref.adam_step — the restatement every optimiser test of the suite goes through — in float64."""
import pytest

import adam_reference as A


@pytest.mark.parametrize("first_step", [1, 5001])
def test_the_restated_adam_step_is_torch_optim_adam_in_float64(first_step):
    worst = max(A.restatement_error(kind, first_step=first_step, betas=betas, eps=eps)
                for kind in A.CLASSES for betas, eps in (((0.9, 0.999), 1e-8), ((0.5, 0.9), 1e-5)))
    assert worst <= 1e-12, worst
