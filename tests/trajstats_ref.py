"""The trajectory sufficient statistics of a batch (csrc/batch_trajstats.hpp, include/cpprob_hip.h: cpprob_hip_batch_traj_stats)
restated in plain Python: the record of one state path and its observes, every accumulator from 0.0 with one IEEE addition a step in
the walk's order t = T-1 .. 0 (Python floats never contract).  The reference of tests/test_trajstats_ref_host.py, the kernel-text
test and tests/test_gpu_batch_trajstats.py, which apply it to tests/backward_ref.py's or Engine.batch_smooth's trajectories."""
import numpy as np

RECORD = 88


def stats(path, obs=None):
    """The statistics of one trajectory x_0 .. x_{T-1} (possibly empty) and its observes: a dict of xi [8, 8] (xi[s][s'], transitions
    s -> s'), occ, occ_y, occ_yy [8]."""
    T = len(path)
    xi = [[0.0] * 8 for _ in range(8)]
    occ, occ_y, occ_yy = [0.0] * 8, [0.0] * 8, [0.0] * 8
    for t in range(T - 1, -1, -1):
        x = int(path[t])
        if t < T - 1:
            xi[x][int(path[t + 1])] = xi[x][int(path[t + 1])] + 1.0
        occ[x] = occ[x] + 1.0
        if obs is not None:
            y = float(obs[t])
            occ_y[x] = occ_y[x] + y
            occ_yy[x] = occ_yy[x] + y * y
    return {"xi": np.array(xi), "occ": np.array(occ), "occ_y": np.array(occ_y), "occ_yy": np.array(occ_yy)}


def record(st):
    """The 88 doubles of a trajectory: xi at 8 s + s', then occ, occ_y, occ_yy."""
    return np.concatenate([st["xi"].reshape(-1), st["occ"], st["occ_y"], st["occ_yy"]])


def records(traj, obs=None):
    """[n_traj, 88]: the records of the columns of traj [T, n_traj]."""
    traj = np.asarray(traj)
    return np.stack([record(stats(traj[:, j], obs)) for j in range(traj.shape[1])]) if traj.shape[1] else np.zeros((0, RECORD))
