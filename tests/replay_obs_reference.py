"""The all-steps observation block of a device replay sample (`mzs_replay_sample_args.obs_steps == k_steps`,
`DeviceReplayBuffer.sample(all_obs=True)`) restated as plain loops: row j is the observations of transitions
start .. start + k - 1 of the drawn episode, element by element; a row with nothing to draw (start -1) is all zeros.
Episodes are the dicts of tests/replay_reference.py; the draws are that module's.  Shares nothing with the kernels."""
import numpy as np

F32 = np.float32


def window_obs(ep, start, k):
    """[k, obs_dim] float32: the observation of every transition of `window(ep, start, k)`."""
    obs_dim = len(ep["obs"][0])
    out = np.zeros((k, obs_dim), F32)
    for i in range(k):
        for c in range(obs_dim):
            out[i][c] = ep["obs"][start + i][c]
    return out


def batch_obs(episodes, e, start, k):
    """[B, k, obs_dim] float32 of the rows (episode index e[j], start[j]); start[j] < 0: a zero-filled row."""
    obs_dim = len(episodes[0]["obs"][0])
    out = np.zeros((len(e), k, obs_dim), F32)
    for j in range(len(e)):
        if int(start[j]) < 0:
            continue
        out[j] = window_obs(episodes[int(e[j])], int(start[j]), k)
    return out
