"""The decision and the chance function of the default stochastic MLP family, composed from the C oracle's own
recurrent_inference (helper, no test functions).  No arithmetic is stated here: each function is two oracle calls with
remapped weight structs --

  * one with that function's dynamics weights in the trio's dynamics places (one-hot width A for the decision function,
    C for the chance function): the next embedding, and for the chance function the reward; its prediction outputs are
    ignored (zero weights);
  * one in recurrent_pred_on = parent mode on the embedding just produced, with that function's two heads in the trio's
    prediction places (head width C for the decision function, A for the chance function): the value and the logits;
    its dynamics weights are zeros of the right shape and its dynamics outputs are ignored.

Weights: a dict of the 28 arrays named as in include/mzsearch.h (mzs_stochastic_mlp_weights), haiku layout w[in][out].
"""
import numpy as np

F32 = np.float32
H = 16
HEADS = ("ad", "av", "ac", "cr", "cn", "pv", "pp")
NAMES = [f"{h}_{a}" for h in HEADS for a in ("w1", "b1", "w2", "b2")]


def head_shapes(A, C, E, F):
    """head -> (inputs, outputs)"""
    return {"ad": (E + A, E), "av": (E, F), "ac": (E, C), "cr": (E + C, F), "cn": (E + C, E), "pv": (E, F), "pp": (E, A)}


def random_weights(seed, A, C, E, support, bias_scale=0.1, scale=1.0):
    """haiku-style init (TruncNormal(1 / sqrt(fan_in))) times `scale`, biases N(0, bias_scale), from a NumPy seed."""
    rng = np.random.default_rng([seed, A, C, E, support])
    w = {}
    for h, (i, o) in head_shapes(A, C, E, 2 * support + 1).items():
        for n, shape in (("w1", (i, H)), ("b1", (H,)), ("w2", (H, o)), ("b2", (o,))):
            if n[0] == "w":
                x = np.clip(rng.standard_normal(shape), -2, 2) * scale / np.sqrt(shape[0])
            else:
                x = bias_scale * rng.standard_normal(shape)
            w[f"{h}_{n}"] = np.ascontiguousarray(x, F32)
    return w


def _trio(oracle, w, dyn_r, dyn_n, pred_v, pred_p, E, width, support, discount, pred_on):
    """An oracle.Mlp whose dynamics are the heads `dyn_r` / `dyn_n` and whose prediction net the heads `pred_v` / `pred_p`
    (None: zeros of the right shape), the one-hot and the policy head `width` wide."""
    F = 2 * support + 1
    z = lambda *s: np.zeros(s, F32)  # noqa: E731

    def head(name, i, o):
        if name is None:
            return z(i, H), z(H), z(H, o), z(o)
        return tuple(w[f"{name}_{a}"] for a in ("w1", "b1", "w2", "b2"))
    ws = {"repr_w": z(1, E), "repr_b": z(E)}
    for pre, name, i, o in (("pv", pred_v, E, F), ("pp", pred_p, E, width), ("dr", dyn_r, E + width, F),
                            ("dn", dyn_n, E + width, E)):
        ws.update(zip((f"{pre}_w1", f"{pre}_b1", f"{pre}_w2", f"{pre}_b2"), head(name, i, o)))
    return oracle.Mlp(ws, 1, E, width, F, discount=discount, support_size=support, recurrent_pred_on=pred_on)


class StochasticMlpReference:
    """decision(action [B], state [B, E]) -> (chance_logits [B, C], afterstate_value [B], afterstate [B, E]);
    chance(outcome [B], afterstate [B, E]) -> (action_logits [B, A], value, reward, discount [B], state [B, E])."""

    def __init__(self, oracle, w, A, C, E, support, discount=0.99):
        self.o, self.A, self.C, self.E = oracle, A, C, E
        t = lambda *a: _trio(oracle, w, *a)  # noqa: E731
        self._d_dyn = t(None, "ad", None, None, E, A, support, discount, 0)
        self._d_pred = t(None, None, "av", "ac", E, C, support, discount, 1)
        self._c_dyn = t("cr", "cn", None, None, E, C, support, discount, 0)
        self._c_pred = t(None, None, "pv", "pp", E, A, support, discount, 1)

    def decision(self, action, state):
        zeros = np.zeros(len(action), np.int32)
        _, _, _, _, after = self.o.recurrent_inference(self._d_dyn, action, state)
        _, _, chance_logits, value, _ = self.o.recurrent_inference(self._d_pred, zeros, after)
        return chance_logits, value, after

    def chance(self, outcome, afterstate):
        zeros = np.zeros(len(outcome), np.int32)
        reward, discount, _, _, state = self.o.recurrent_inference(self._c_dyn, outcome, afterstate)
        _, _, action_logits, value, _ = self.o.recurrent_inference(self._c_pred, zeros, state)
        return action_logits, value, reward, discount, state

    def row(self, slot, parent_embedding):
        """Both functions on all rows at the clamped slots, as StochasticScript.row orders them (what search_stochastic
        evaluates and StochasticStepper.expand_backup takes)."""
        slot = np.asarray(slot, np.int32)
        cl, av, ae = self.decision(np.clip(slot, 0, self.A - 1), parent_embedding)
        al, v, r, d, se = self.chance(np.clip(slot - self.A, 0, self.C - 1), parent_embedding)
        return (cl, av), ae, (al, v, r, d), se
