"""Reference of the stochastic family's forward value unroll (mzs_stochastic_mlp_unroll_values /
MuZero.unroll_values on an SMZNetwork), shared by test_stochastic_unroll_cpu.py and
test_gpu_stochastic_unroll.py (helper, no test functions).

`oracle_chain` is composed from the C oracle's root_inference / recurrent_inference alone, with remapped weight structs
as tests/stochastic_mlp_reference.py remaps them -- no arithmetic is stated here:

  * root_inference on a trio holding repr_* and pv: v_0 and s_0;
  * the afterstate dynamics `ad` in the trio's next-state place, one-hot width A: after_i;
  * the encoder in recurrent_pred_on = parent mode with en_* in the policy head's place, E := obs_dim, width := C and
    the raw observation row as the "embedding": a bare Linear-elu-Linear, the C logits; the code is np.argmax (the first
    maximum);
  * the chance dynamics `cn` in the trio's next-state place, one-hot width C: s_{i+1};
  * recurrent_pred_on = parent mode on s_{i+1} with pv in the value head's place: v_{i+1}.

An action outside 0..A-1 (for the kernel the all-zero one-hot) is given to the oracle as action A of a net with A + 1
actions whose extra ad_w1 row is zero, as tests/unroll_reference.py does: one more link fma(1, 0, acc) at the end of the
k-ordered chain, which changes no bit of a non-zero sum (the cases use non-zero biases).

Weights: a dict of the 34 arrays named as in include/mzsearch.h (mzs_stochastic_train_weights), haiku layout w[in][out]."""
import numpy as np

import stochastic_mlp_reference as smref

F32 = np.float32
H = smref.H


def random_weights(seed, A, C, E, support, obs_dim, bias_scale=0.1):
    """The 34 arrays: smref.random_weights' 28, and the representation and the encoder by the same rule."""
    w = smref.random_weights(seed, A, C, E, support, bias_scale=bias_scale)
    rng = np.random.default_rng([seed, A, C, E, support, obs_dim])
    for n, shape in (("repr_w", (obs_dim, E)), ("repr_b", (E,)), ("en_w1", (obs_dim, H)), ("en_b1", (H,)),
                     ("en_w2", (H, C)), ("en_b2", (C,))):
        if n[-2] == "w" or n == "repr_w":
            x = np.clip(rng.standard_normal(shape), -2, 2) / np.sqrt(shape[0])
        else:
            x = bias_scale * rng.standard_normal(shape)
        w[n] = np.ascontiguousarray(x, F32)
    return w


def make_case(A, C, E, support, obs_dim, B, L, seed=None, bias_scale=0.1):
    """Seeded weights, observations [B, L, obs_dim], actions and returns of one shape."""
    seed = 1000 * A + 100 * C + 10 * E + support if seed is None else seed
    rng = np.random.default_rng(seed + 7)
    return dict(w=random_weights(seed, A, C, E, support, obs_dim, bias_scale), A=A, C=C, E=E, support=support,
                obs_dim=obs_dim, B=B, L=L, obs=rng.uniform(-1, 1, (B, L, obs_dim)).astype(F32),
                a=rng.integers(0, A, (B, L)).astype(np.int32), Rn=rng.uniform(-30, 60, (B, L)).astype(F32))


def model_weights(model):
    """The 34 arrays of a model on the default stochastic MLP family, as host float32 arrays."""
    import muax_amd as mx
    return {n: x.detach().cpu().numpy().astype(F32) for n, x in mx.nn.stochastic_train_weights(model.network).items()}


def encoder_logits(oracle, w, obs_rows, C, support):
    """en(obs_rows) [B, C] on the oracle: the encoder in the policy head's place of a parent-mode recurrent call."""
    obs_rows = np.ascontiguousarray(obs_rows, F32)
    enc = smref._trio(oracle, w, None, None, None, "en", obs_rows.shape[1], C, support, 0.99, 1)
    _, _, logits, _, _ = oracle.recurrent_inference(enc, np.zeros(len(obs_rows), np.int32), obs_rows)
    return logits


def oracle_chain(oracle, w, obs, a, Rn, A, C, E, support, kp):
    """(values [B, kp] float32, prio [B, kp] float32, codes [B, kp] int32 with -1 in column 0).
    obs: [B, L, obs_dim]; a, Rn: [B, L]; L >= kp."""
    obs, a, Rn = np.asarray(obs, F32), np.asarray(a, np.int64), np.asarray(Rn, F32)
    B, _, obs_dim = obs.shape
    F = 2 * support + 1
    used = a[:, :kp - 1]
    if ((used < 0) | (used >= A)).any():  # the zero-row net: action A contributes nothing
        w = dict(w)
        w["ad_w1"] = np.concatenate([np.asarray(w["ad_w1"], F32), np.zeros((1, H), F32)], 0)
        a, A = np.where((a < 0) | (a >= A), A, a), A + 1
    zeros = np.zeros(B, np.int32)
    pred = smref._trio(oracle, w, None, None, "pv", None, E, A, support, 0.99, 1)
    root_w = dict(pred.w, repr_w=w["repr_w"], repr_b=w["repr_b"])
    root = oracle.Mlp(root_w, obs_dim, E, A, F, support_size=support, recurrent_pred_on=0)
    after_dyn = smref._trio(oracle, w, None, "ad", None, None, E, A, support, 0.99, 0)
    chance_dyn = smref._trio(oracle, w, None, "cn", None, None, E, C, support, 0.99, 0)
    values, codes = np.zeros((B, kp), F32), np.full((B, kp), -1, np.int32)
    _, values[:, 0], s = oracle.root_inference(root, obs[:, 0])
    for i in range(kp - 1):
        _, _, _, _, after = oracle.recurrent_inference(after_dyn, a[:, i], s)
        codes[:, i + 1] = np.argmax(encoder_logits(oracle, w, obs[:, i + 1], C, support), axis=1)
        _, _, _, _, s = oracle.recurrent_inference(chance_dyn, codes[:, i + 1], after)
        _, _, _, values[:, i + 1], _ = oracle.recurrent_inference(pred, zeros, s)
    with np.errstate(invalid="ignore"):
        return values, np.abs(values - Rn[:, :kp]).astype(F32), codes


def bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)
