"""GPU: pyoak.BuildTrajectories / pyoak.read_build_trajectories, the reference's names (cpp/src/pyoak.cc:247-329, 697-715) over the device
reader: the reference's seven fields in its shapes, every row the referee's decode of one record of the files, and the prelude of
build.py's process_targets (src/oak/build.py:157-195, as written there) running on them."""
import numpy as np
import pytest
import torch

import build_traj_ref as T

pytestmark = pytest.mark.gpu


def _get_state(actions):
    b, T_, _ = actions.shape
    state = torch.zeros((b, T_, T.N_DIM + 1), dtype=torch.float32)
    state = state.scatter(2, actions + 1, 1.0)
    state = torch.cumsum(state, dim=1).clamp_max(1.0)
    state = state[:, :-1, 1:]
    return torch.concat([torch.zeros(state[:, :1].shape), state], dim=1)


def test_read_build_trajectories_and_the_prelude_of_process_targets(gpu_ctx, tmp_path):
    from oak_amd import build, pyoak
    records = T.rollout_records(90, 11, zero_prob=0.0)
    ref = T.decode_many(records)
    assert (ref["status"] == T.OK).all()
    paths = []
    for k, (lo, hi) in enumerate(((0, 50), (50, 57), (57, 90))):
        paths.append(str(tmp_path / ("%d.build.data" % k)))
        open(paths[-1], "wb").write(records[lo:hi].tobytes())
    size = 64
    traj = pyoak.BuildTrajectories(size)
    shapes = {"action": (size, 31, 1), "policy": (size, 31, 1), "mask": (size, 31, 339), "value": (size, 1), "score": (size, 1), "start": (size, 1), "end": (size, 1)}
    for name, shape in shapes.items():
        assert getattr(traj, name).shape == shape
    assert traj.mask.dtype == np.int64 and traj.action.dtype == np.int64 and traj.policy.dtype == np.float32 and traj.end.dtype == np.int64
    assert pyoak.read_build_trajectories(traj, paths, 4) == size
    assert (traj.status == 0).all()
    by_key = {(ref["action"][r].tobytes(), ref["policy"][r].tobytes(), float(ref["value"][r])): r for r in range(len(records))}
    seen = set()
    for row in range(size):
        r = by_key[(traj.action[row].tobytes(), traj.policy[row].tobytes(), float(traj.value[row, 0]))]
        seen.add(r)
        assert np.array_equal(traj.mask[row], ref["mask"][r]) and traj.score[row, 0] == ref["score"][r]
        assert traj.start[row, 0] == ref["start"][r] and traj.end[row, 0] == ref["end"][r]
    assert len(seen) > 20 and min(seen) < 50 <= max(seen)            # draws over more than one file
    # the prelude of process_targets, as build.py writes it
    action, policy, mask = torch.from_numpy(traj.action), torch.from_numpy(traj.policy), torch.from_numpy(traj.mask)
    value, score, end = torch.from_numpy(traj.value), torch.from_numpy(traj.score), torch.from_numpy(traj.end)
    t_max = torch.max(end).item()
    valid = torch.logical_and(action != -1, policy > 0).squeeze(-1)
    valid_state = _get_state(action)[valid]
    valid_mask = mask[valid]
    valid_old_logp = torch.log(policy[valid])
    value_weight = 0.6
    r = value_weight * value + (1 - value_weight) * score
    rewards = torch.zeros_like(policy).scatter(1, end.unsqueeze(-1) - 1, r.unsqueeze(-1))
    assert 0 < t_max <= 31 and valid_state.shape == (int(valid.sum()), T.N_DIM) and valid_mask.shape == (int(valid.sum()), 339)
    assert bool((valid_mask[:, 0] == action.squeeze(-1)[valid]).all())
    # ... and the device's own targets from the same arrays say the same
    decoded = {"action": traj.action[:, :, 0], "policy": traj.policy[:, :, 0], "value": traj.value[:, 0], "score": traj.score[:, 0],
               "start": traj.start[:, 0], "end": traj.end[:, 0]}
    got = build.targets(gpu_ctx, decoded, value_weight)
    assert np.array_equal(got["valid"], valid.numpy()) and np.array_equal(got["rewards"], rewards.squeeze(-1).numpy())
    assert np.array_equal(build.dense_state(gpu_ctx, got, 0, got["n_valid"]), valid_state.numpy())
    assert np.abs(got["old_logp"] - valid_old_logp.numpy()[:, 0]).max() <= 2e-6    # (torch's float log is no referee: 1.5 ulp at |x| < 16, a sanity check)
    # a refusal gives 0, as the reference's reader does
    bad = str(tmp_path / "bad.build.data")
    open(bad, "wb").write(records[:2].tobytes()[:-1])
    assert pyoak.read_build_trajectories(traj, [paths[0], bad], 1) == 0
