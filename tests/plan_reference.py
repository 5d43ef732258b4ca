"""The episode plan of a collection call (mzs_replay_plan_steps, include/mzsearch.h) as a plain loop over Python ints
and floats, written from the arithmetic the header states.  It shares no code with muax_amd/vector.py: the CPU tests
hold it against `vector.ring_plan` and collect()'s returns, the GPU tests hold the kernels against it."""


def plan_steps(done, r, row0, steps, ring_steps, open_len, open_ret, min_length):
    """done, r: [ring_steps][N] nested sequences (flags, rewards), indexed by RING row.  open_len, open_ret: [N].
    Returns (ep, ret, counts, new open_len, new open_ret): ep the rows (environment, first ring row, length, stored),
    environment-major then time, ret their returns, counts = [episodes, stored episodes, max new open_len, 0]."""
    S, N = int(ring_steps), len(open_len)
    ep, ret, new_len, new_ret = [], [], [], []
    for e in range(N):
        length, g = int(open_len[e]), float(open_ret[e])
        first = ((row0 - int(open_len[e]) % S) + S) % S
        for t in range(steps):
            row = (row0 + t) % S
            length += 1
            g = g + float(r[row][e])
            if done[row][e]:
                ep.append((e, first, length, 1 if length >= min_length else 0))
                ret.append(g)
                first = (row + 1) % S
                length, g = 0, 0.0
        new_len.append(length)
        new_ret.append(g)
    counts = [len(ep), sum(x[3] for x in ep), max(new_len), 0]
    return ep, ret, counts, new_len, new_ret
