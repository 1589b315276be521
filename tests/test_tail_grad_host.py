"""The float64 side of tests/test_gpu_differentiable.py on the CPU: the step size the device's gradient descent is given was
chosen here, with a factor of two to spare."""
from tests import tail_grad_ref as T


def test_float64_descent_is_monotone_at_the_step_size_and_at_twice_it():
    for lr in (T.DESCENT_LR, 2 * T.DESCENT_LR):
        losses = T.descend64(lr)
        print(lr, ['%.6g' % v for v in losses])
        assert len(losses) == T.DESCENT_STEPS + 1 and all(b < a for a, b in zip(losses, losses[1:])), (lr, losses)
    # ... and each step moves the loss by far more than fp32 can blur it (2^-24 relative per value)
    losses = T.descend64(T.DESCENT_LR)
    assert min(a - b for a, b in zip(losses, losses[1:])) > 1e-3 * losses[0]


def test_every_term_reaches_the_state():
    state, camera, gt = T.problem()
    _, g = T.grad64({k: v.astype('float64') for k, v in state.items()}, camera, gt, T.WEIGHTS)
    assert all(abs(v).max() > 0 for v in g.values()) and g['x6d'].shape == (T.B, 144)
