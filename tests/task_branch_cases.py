"""The tables whose branches tests/test_task_branches_cpu.py counts, run in this process: what that test starts as a child with the
emulator built under --coverage.  The kernels between two rigid-body steps (chain_kernels.hip, reset_kernels.hip, task_kernels.hip,
task_device.h, traj_kernels.hip, order_device.h, locoval_returns_device.h) are reached through

    tests/chain_cases.py        the pooled reset / observation launch                  (test_chain_cpu.py)
    tests/reset_cases.py        the reset conformance matrix                           (test_reset_matrix_cpu.py)
    tests/task_cases.py         the post-physics conformance matrix                    (test_task_matrix_cpu.py)
    tests/obs_pass_cases.py     one observation pass per step                          (test_obs_pass_once_cpu.py)
    the waypoint densifier's table                                                     (test_traj_densify_cpu.py)
    the task, flags, compaction, order and trajectory tests of test_emu_kernels.py     (not its rigid-body, GEMM, attention, PPO tests)
    the rollout's LocoVal return bookkeeping, staged rewards included                  (test_locoval_rollout_cpu.py)

each with its own assertions (float64, the oracle, bit equality): a table that fails here fails the gate.  `--skip EXPR` leaves out the
tests whose id matches the pytest -k expression EXPR (to see which line a case alone takes), e.g. --skip "still and root"."""
import os
import sys

FILES = ("test_chain_cpu.py", "test_reset_matrix_cpu.py", "test_task_matrix_cpu.py", "test_obs_pass_once_cpu.py", "test_traj_densify_cpu.py",
         "test_emu_kernels.py", "test_locoval_rollout_cpu.py")
NOT_BETWEEN_STEPS = ("sim_step", "sim_fk", "gemm", "attention", "softmax", "column_sum", "adam", "locoval_kernels", "obs_normalize", "rms_update",
                     "feed_forward", "ppo_loss", "gather_flat", "act_bwd", "disc_reward", "return_accumulator", "fit_grad", "rollout_targets",
                     "cosine_schedule", "two_rank")


def main(argv):
    import pytest
    here = os.path.dirname(os.path.abspath(__file__))
    skip = [argv[i + 1] for i, a in enumerate(argv) if a == "--skip"]
    expr = " and ".join([f"not {w}" for w in NOT_BETWEEN_STEPS] + [f"not ({s})" for s in skip])
    return pytest.main(["-q", "-x", "-p", "no:cacheprovider", "-p", "no:xdist", "-k", expr] + [os.path.join(here, f) for f in FILES])


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.exit(main(sys.argv[1:]))
