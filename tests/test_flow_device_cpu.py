"""CPU checks of the registration from a problem's own observations (include/srmap.h: srmap_problem_register_flow) through
its numpy restatement (tests/data_prior_restatement.py: plane_of, problem_register_flow over
tests/flow_registration_restatement.py): which plane is registered, and how hr_scale is handled.
tests/test_gpu_flow_device.py compares the GPU against the same rules."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import data_prior_restatement as dp  # noqa: E402
import flow_registration_restatement as fq  # noqa: E402
import test_flow_registration_cpu as cpu  # noqa: E402


@pytest.fixture(scope="module")
def stack3():
    """3 frames of 3 channels at 17 x 23: the deformed stack with a gain per channel and a little noise."""
    rng = np.random.default_rng(12)
    stack = cpu.deformed_stack(17, 23, 3)
    return np.stack([stack * (1.0 - 0.15 * c) + 0.01 * rng.standard_normal(stack.shape) for c in range(3)], axis=1)


def test_the_plane_rule(stack3):
    y = stack3
    for c in range(3):
        flow, prior, q = dp.problem_register_flow(y, c, 2)
        ref = fq.register_flow(y[:, c], hr_scale=2)
        assert np.array_equal(flow, ref[0]) and np.array_equal(q, ref[2])
        assert np.array_equal(prior, np.broadcast_to(ref[1][:, None], y.shape))
    # the mean: the sum in ascending channel order, one division by C -- not numpy's pairwise mean, not a product by 1 / C
    mean = ((y[:, 0] + y[:, 1]) + y[:, 2]) / 3.0
    assert np.array_equal(dp.plane_of(y, -1), mean)
    flow, prior, q = dp.problem_register_flow(y, -1, 2)
    ref = fq.register_flow(mean, hr_scale=2)
    assert np.array_equal(flow, ref[0]) and np.array_equal(q, ref[2])
    other = (y[:, 2] + y[:, 1] + y[:, 0]) * (1.0 / 3.0)
    assert not np.array_equal(other, mean)
    # f32 observations convert exactly, and the field is rounded once
    y32 = y.astype(np.float32)
    flow32, _, q32 = dp.problem_register_flow(y32, -1, 2, dtype=np.float32)
    ref32 = fq.register_flow(dp.plane_of(y32.astype(np.float64), -1), hr_scale=2)
    assert np.array_equal(flow32, ref32[0].astype(np.float32).astype(np.float64)) and np.array_equal(q32, ref32[2])
    assert not np.array_equal(flow32, ref32[0])
    assert np.all(prior[0] == 1) and np.any(prior[1:] == 0)


def test_hr_scale_is_one_or_the_problems(stack3):
    y = stack3
    a = dp.problem_register_flow(y, 0, 3)
    b = dp.problem_register_flow(y, 0, 3, hr_scale=3)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    assert a[0].shape == (3, 2, 51, 69)
    for bad in (0, 2, 4):
        with pytest.raises(fq.FlowRegistrationError):
            dp.problem_register_flow(y, 0, 3, hr_scale=bad)
    for channel in (3, -2):
        with pytest.raises(fq.FlowRegistrationError):
            dp.problem_register_flow(y, channel, 3)
    with pytest.raises(fq.FlowRegistrationError):
        dp.problem_register_flow(np.zeros((0, 1, 17, 23)), 0, 2)
    with pytest.raises(fq.FlowRegistrationError):
        dp.problem_register_flow(np.zeros((2, 1, 15, 23)), 0, 2)
