"""No GPU: the conditions under which the oracle comparison of tests/test_gpu_ddp.py means something, checked on the CPU
oracle alone (tests/ddp_cases.py).

  * a wrong exchange is far outside the fp32 noise of the right one: global BatchNorm statistics, rank 0's gradient alone and
    a sum instead of a mean each lie at least 20 times farther from the fp64 two-replica mean gradient than the same step
    computed in CPU fp32 does, at the median over the parameter tensors (measured: more than 100 times, errors near 1);
  * rank 1's running statistics differ from rank 0's by more than 10 % of the size of rank 0's own update (measured: 246 % in
    the worst BatchNorm layer, 11 % at the median), and are not allclose to them at 100 times the tolerance the GPU test grants,
    so "every rank holds rank 0's" cannot pass by accident;
  * the two ranks' initial weights differ, so the initial broadcast matters."""
import pytest
import torch

import ddp_cases as D


@pytest.fixture(scope="module")
def steps():
    s64 = D.two_replica_step(torch.float64)
    return s64, D.two_replica_step(torch.float32)


def test_wrong_exchanges_lie_far_outside_the_fp32_noise(steps):
    s64, s32 = steps
    med32, p90_32, max32 = D.quantiles(D.tensor_errs(s32["mean_grad"], s64["mean_grad"]))
    print("cpu fp32 two-replica mean vs fp64: median %.3g p90 %.3g max %.3g" % (med32, p90_32, max32))
    assert 0 < med32 < 5e-2     # fp32 noise through 46 training-mode BatchNorms, not a different computation
    for name, g in D.wrong_variants(s64).items():
        med, p90, mx = D.quantiles(D.tensor_errs(g, s64["mean_grad"]))
        print("%s vs fp64 two-replica mean: median %.3g p90 %.3g max %.3g (%.0fx fp32)" % (name, med, p90, mx, med / med32))
        assert med >= 20 * med32, (name, med, med32)


def test_rank_1_running_statistics_differ_from_rank_0(steps):
    s64, _ = steps
    gap = D.running_stat_gap(s64["buffers"])
    assert len(gap) == 2 * 46   # running_mean and running_var of every BatchNorm
    med, p90, mx = D.quantiles(gap)
    print("rank 1 vs rank 0 running statistics, relative to rank 0's update: median %.3g p90 %.3g max %.3g" % (med, p90, mx))
    assert mx > 0.10, (med, p90, mx)
    cat = lambda b: torch.cat([v.flatten() for k, v in b.items() if not k.endswith("num_batches_tracked")])
    # the GPU test compares with rtol 1e-4, atol 1e-5: rank 1's statistics fail that with two orders of magnitude to spare
    assert not torch.allclose(cat(s64["buffers"][1]), cat(s64["buffers"][0]), rtol=1e-2, atol=1e-3)


def test_ranks_start_from_different_weights_and_batches():
    a, b = D.initial_model(0).state_dict(), D.initial_model(1).state_dict()
    assert any(not torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(D.batch(0)[0], D.batch(1)[0]) and not torch.equal(D.batch(0)[1], D.batch(1)[1])
    assert D.batch(0)[0].shape == (2, 5, 96, 128) and D.batch(0)[1].dtype == torch.uint8
