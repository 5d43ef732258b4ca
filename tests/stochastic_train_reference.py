"""The fused stochastic training step's reference (test_stochastic_train_cpu.py, test_gpu_stochastic_train.py): torch
autograd through loss.stochastic_loss_fn on a copy of the model's six modules, float64 on the CPU by default.  The loss's
own `t()` casts every batch field to the modules' dtype, so the float64 copy evaluates the whole formula in float64.

`conditions()` measures, in float64, how far the inputs are from the places where float32 and float64 may legitimately
take different branches: the encoder's top-two logit gap (the argmax), the gap between the two smallest and between the
two largest inputs of every min_max_normalize (the tie rule), the distance of every scaled support target from an
integer (floor / ceil)."""
import copy

import numpy as np
import torch

from helpers import train_batch

F32 = np.float32

# (A, C, E, support, obs_dim) of the GPU tests: every vector in one slot and C < A; X = E + C = 48, chance logits in two
# slots, E + A across a slot boundary; C and obs_dim just past a slot boundary
SHAPES = [(3, 2, 4, 8, 5), (4, 32, 16, 10, 16), (4, 17, 8, 8, 20)]


def smz_model(A, Cn, E, support, obs_dim, seed, device=None, bias_noise=True, optimizer=("adam", 1e-2), **model_kw):
    """A default stochastic MLP family with haiku's init; `bias_noise` adds N(0, 0.1) to every bias so that every bias
    path carries a gradient.  The weights do not depend on the device (CPU generator)."""
    import muax_amd as mx
    g = torch.Generator().manual_seed(seed)
    net = mx.create_stochastic_muzero_network(E, A, Cn, 2 * support + 1, generator=g)
    m = mx.MuZero(net, optimizer=mx.optimizers.create_optimizer(*optimizer), support_size=support, device=device, **model_kw)
    m.init(0, np.zeros((1, obs_dim)))
    if bias_noise:
        with torch.no_grad():
            for p in [p for mod in m.network for p in mod.parameters()]:
                if p.dim() == 1:
                    p.add_(0.1 * torch.randn(p.shape, generator=g).to(p.device))
        m.weights_changed()
    return m


def smz_batch(B, L, A, obs_dim, seed):
    """obs [B, L, obs_dim] in (-1, 1), r in (-2, 3), Rn in (-30, 60) (inside the clip of support 8), Dirichlet pi."""
    return train_batch(B, L, A, obs_dim, seed)


def cut_rows(b, rows):
    import muax_amd as mx
    return mx.Transition(**{k: (np.asarray(v)[rows] if np.ndim(v) else v) for k, v in b.__dict__.items()})


def copy_model(m, dtype=torch.float64, device="cpu"):
    import muax_amd as mx
    mods = [copy.deepcopy(x).to(device=device, dtype=dtype) for x in m.network]
    m2 = mx.MuZero(mx.nn.SMZNetwork(*mods), device=device, support_size=m._support_size)
    m2._params = True
    return m2


def autograd(m, b, dtype=torch.float64, device="cpu", **kw):
    """(loss, [gradient of every STOCHASTIC_TRAIN_WEIGHT_NAMES array] as float64 NumPy) of loss.stochastic_loss_fn."""
    import muax_amd as mx
    from muax_amd._lib import STOCHASTIC_TRAIN_WEIGHT_NAMES
    m2 = copy_model(m, dtype, device)
    loss = mx.loss.stochastic_loss_fn(m2, b, **kw)
    assert loss.dtype == dtype
    loss.backward()
    w = mx.nn.stochastic_train_weights(m2.network)
    return float(loss.detach()), [w[n].grad.detach().cpu().double().numpy() for n in STOCHASTIC_TRAIN_WEIGHT_NAMES]


def conditions(m, b):
    """float64, per (row, step) or finer: dict(encoder_gap [B, L-1], minmax_gap [B, 2 L - 1] (the representation's, then
    the afterstate's and the next state's of every transition; the smaller of bottom-two and top-two gap),
    target_distance [B, 2 L] (r, then Rn))."""
    import muax_amd as mx
    m2 = copy_model(m)
    B, L = np.asarray(b.a).shape[:2]
    obs = torch.as_tensor(np.asarray(b.obs), dtype=torch.float64)
    with torch.no_grad():
        gaps = []
        for i in range(1, L):
            top = m2.enc_func(obs[:, i]).topk(2, dim=-1).values
            gaps.append((top[:, 0] - top[:, 1]).numpy())
        cap = []
        norm = mx.nn.min_max_normalize

        def recording(s):
            cap.append(s.detach().clone())
            return norm(s)
        mx.nn.min_max_normalize = recording
        try:
            mx.loss.stochastic_loss_fn(m2, b)
        finally:
            mx.nn.min_max_normalize = norm
    assert len(cap) == 2 * L - 1
    mm = []
    for u in cap:
        u = u.sort(dim=1).values
        mm.append(torch.minimum(u[:, 1] - u[:, 0], u[:, -1] - u[:, -2]).numpy())
    S = m._support_size
    x = np.concatenate([np.asarray(b.r, np.float64).reshape(B, L), np.asarray(b.Rn, np.float64).reshape(B, L)], 1)
    xs = np.clip(np.sign(x) * (np.sqrt(np.abs(x) + 1) - 1) + 1e-3 * x, -S, S)
    return dict(encoder_gap=np.stack(gaps, 1) if gaps else np.zeros((B, 0)), minmax_gap=np.stack(mm, 1),
                target_distance=np.abs(xs - np.round(xs)))


def well_conditioned(cond):
    enc, mm, td = cond["encoder_gap"], cond["minmax_gap"], cond["target_distance"]
    return (enc.size == 0 or enc.min() >= 1e-3) and mm.min() >= 1e-4 and td.min() >= 1e-4


def rel_errors(got, ref):
    """max |got - ref| per array over max(largest |ref| entry, 1e-6): the measure of tests/test_gpu_train.py"""
    return [float(np.abs(np.asarray(g, np.float64) - d).max() / max(np.abs(d).max(), 1e-6)) for g, d in zip(got, ref)]
