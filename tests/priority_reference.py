"""Plain-loop NumPy statement of the priority write-back (mzs_replay_update_priorities), for
test_priority_cpu.py and test_gpu_priority.py.  Rows are applied in ascending j, element by element, a later valid
element overwriting an earlier one (NumPy's w[idx] = p); then every episode that received at least one valid element
gets the sequential prefix sum of its weights and its table weight.  Nothing here is vectorised over rows."""
import numpy as np


def update(w, cw, t_w, live, serial, start, prio, alpha=1.0, eps=0.0, weight="mean"):
    """`w`, `cw` [max_steps] and `t_w` [capacity] float64 (not modified); `live`: (slot, first row, length, serial) of
    every live episode; `serial` [B], `start` [B], `prio` [B] or [B, kp].  Returns (w, cw, t_w, slots) -- new arrays
    and the set of table slots of the episodes that were written.

    Skipped: a row whose serial is not live, a row with start < 0, an element at or past the episode's end, an
    element whose priority is NaN or infinite."""
    assert weight in ("mean", "sum")
    w, cw, t_w = (np.array(x, np.float64) for x in (w, cw, t_w))
    serial, start = np.asarray(serial).reshape(-1), np.asarray(start).reshape(-1)
    prio = np.asarray(prio, np.float32).reshape(len(serial), -1)
    by_serial = {int(s): (int(slot), int(first), int(T)) for slot, first, T, s in live}
    written = {}
    for j in range(len(serial)):
        ep = by_serial.get(int(serial[j]))
        if ep is None or int(start[j]) < 0:
            continue
        slot, first, T = ep
        for i in range(prio.shape[1]):
            t, p = int(start[j]) + i, prio[j, i]
            if t >= T or not np.isfinite(p):
                continue
            w[first + t] = (abs(np.float64(p)) + eps) ** alpha
            written[slot] = (first, T)
    for slot, (first, T) in written.items():
        cw[first:first + T] = np.cumsum(w[first:first + T])
        t_w[slot] = cw[first + T - 1] / T if weight == "mean" else cw[first + T - 1]
    return w, cw, t_w, set(written)
