"""References of the forward value unroll (mzs_mlp_unroll_values / MuZero.unroll_values), shared by
test_unroll_values_cpu.py and test_gpu_unroll_values.py.

`oracle_chain`: the arithmetic spec itself, per row on the C oracle -- root_inference gives v_0 and the embedding, then
recurrent_inference(mlp, a_i, emb) with recurrent_pred_on=0 gives v_{i+1} and the next embedding; p = |v - Rn| in
float32.  The kernel is held to its bits.  An action outside 0..A-1 (for the kernel the all-zero one-hot) is given to the
oracle as action A of a net with A + 1 actions whose extra dn_w1 / dr_w1 row and extra pp_w2 column are zero: one more
link `acc = fma(1, 0, acc)` at the end of the k-ordered chain, which changes no bit of a non-zero sum (the cases use
non-zero biases, so the sign of a zero cannot matter), and for every other action one more `fma(0, 0, acc)`.

`fp64_chain`: the float64 restatement built from oracle/mz_train_numpy.forward(trace=): its "states", then
_mlp(w, "pv", s), softmax, expectation over the support and the inverse of h."""
import numpy as np

F32 = np.float32


def make_case(oracle, A, E, support, obs_dim, B, L, seed=None, bias_scale=0.1):
    """Seeded weights (haiku's init, biases N(0, bias_scale)), observations, actions and returns of one shape."""
    seed = 1000 * A + 10 * E + support if seed is None else seed
    w = oracle.random_mlp_weights(seed, obs_dim, E, A, 2 * support + 1, bias_scale=bias_scale)
    rng = np.random.default_rng(seed + 7)
    return dict(w=w, A=A, E=E, support=support, obs_dim=obs_dim, B=B, L=L,
                obs=rng.uniform(-1, 1, (B, obs_dim)).astype(F32), a=rng.integers(0, A, (B, L)).astype(np.int32),
                Rn=rng.uniform(-30, 60, (B, L)).astype(F32))


def _zero_row_net(w, A):
    """The net with A + 1 actions whose action A contributes nothing."""
    w = {k: np.array(v, F32) for k, v in w.items()}
    for k in ("dn_w1", "dr_w1"):
        w[k] = np.concatenate([w[k], np.zeros((1, w[k].shape[1]), F32)], 0)
    w["pp_w2"] = np.concatenate([w["pp_w2"], np.zeros((w["pp_w2"].shape[0], 1), F32)], 1)
    w["pp_b2"] = np.concatenate([w["pp_b2"], np.zeros(1, F32)])
    return w


def oracle_chain(oracle, w, obs, a, Rn, support, kp):
    """(values, prio), both [B, kp] float32.  a, Rn: [B, L] with L >= kp."""
    obs, a, Rn = np.asarray(obs, F32), np.asarray(a, np.int64), np.asarray(Rn, F32)
    obs_dim, E = w["repr_w"].shape
    A = w["pp_b2"].shape[0]
    used = a[:, :kp - 1]
    if ((used < 0) | (used >= A)).any():
        w, a = _zero_row_net(w, A), np.where((a < 0) | (a >= A), A, a)
        A += 1
    mlp = oracle.Mlp(w, obs_dim, E, A, 2 * support + 1, support_size=support, recurrent_pred_on=0)
    B = obs.shape[0]
    values = np.zeros((B, kp), F32)
    _, values[:, 0], emb = oracle.root_inference(mlp, obs)
    for i in range(kp - 1):
        _, _, _, values[:, i + 1], emb = oracle.recurrent_inference(mlp, a[:, i], emb)
    with np.errstate(invalid="ignore"):
        return values, np.abs(values - Rn[:, :kp]).astype(F32)


def _inv_h(y, eps=1e-3):
    """The inverse of h(x) = sign(x) (sqrt(|x| + 1) - 1) + eps x (muax/utils.py:70-76), float64."""
    return np.sign(y) * (((np.sqrt(1.0 + 4.0 * eps * (np.abs(y) + 1.0 + eps)) - 1.0) / (2.0 * eps)) ** 2 - 1.0)


def fp64_chain(w, obs, a, Rn, support, kp):
    """(values, prio), both [B, kp] float64: the unroll on the float32 weights and inputs in float64 throughout."""
    from oracle import mz_train_numpy as ref
    a = np.asarray(a)[:, :kp]
    B, A = a.shape[0], w["pp_b2"].shape[0]
    w64 = {n: np.asarray(w[n], np.float64) for n in ref.WEIGHT_NAMES}
    trace = {}
    ref.forward(w64, obs, a, np.zeros((B, kp)), np.zeros((B, kp)), np.full((B, kp, A), 1.0 / A), support, trace=trace)
    bins = np.arange(-support, support + 1, dtype=np.float64)
    values = np.zeros((B, kp))
    for i, s in enumerate(trace["states"]):
        logits, _ = ref._mlp(w64, "pv", s)
        e = np.exp(logits - logits.max(1, keepdims=True))
        values[:, i] = _inv_h((e / e.sum(1, keepdims=True)) @ bins)
    return values, np.abs(values - np.asarray(Rn, np.float64)[:, :kp])


def bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)
