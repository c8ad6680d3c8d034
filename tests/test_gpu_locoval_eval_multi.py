"""GPU: several LocoVal networks scored on the same games in one evaluation (`run.py --test --compare_valuenet`) on the MI355X.

  (a) the raw C ABI: emloco_locoval_eval_fwd_multi against the networks' own forward-rows, bit for bit, on a mask with holes;
  (b) the value planes against float64 torch at the bar tests/test_gpu_locoval_variants.py holds for these networks (its inputs, its
      networks, its measure: `_float64_errors` there);
  (c) `run.py --test` with three checkpoints beside three single runs: reports and records equal bit for bit;
  (d) the per-step LocoVal part (step + forward + finish) of four networks through the new path against the four passes of the
      existing three launches it replaces, timed on events in one process; the figures go to the file EMLOCO_LOCOVAL_EVAL_MULTI_TABLE
      names (profiles/locoval_eval_multi.txt).
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from locoval_harness import DIMS, _ptr as P, eval_state  # noqa: E402
from test_gpu_locoval_variants import TorchVariantNet, _embed_in_full, _net  # noqa: E402
from test_locoval_variants_cpu import VARIANTS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV_ARGS = ["--random_heading", "--init_heading", "--heading_inversion", "--adjust_root_vel"]
DEV = "cuda:0"


def _weights(net):
    n = net._network
    return [n.fc1.weight, n.fc1.bias, n.fc2.weight, n.fc2.bias, n.fc3.weight, n.fc3.bias]


def _inputs(B, seed):
    """the inputs of tests/test_gpu_locoval_variants.py:_float64_errors"""
    g = torch.Generator().manual_seed(seed)
    traj = torch.cumsum(torch.randn(B, 13, 3, generator=g) * 0.3 + torch.tensor([0.5, 0.1, 0.0]), dim=1)
    traj[:, 0] = 0
    pose, vel = torch.randn(B, 24, 3, generator=g) * 0.3, torch.randn(B, 2, generator=g)
    return traj.to(DEV).contiguous(), pose.to(DEV).contiguous(), vel.to(DEV).contiguous()


def _state(B, traj, pose, vel, mask):
    """an EmlocoLocoValEval that carries what the forward reads: the staged inputs and the row mask"""
    from emloco_amd.predictor import ops
    s = ops.LocoValEval(n_env=B, step_to_pred=5, games_per_env=1, gamma=0.99)
    s.traj13, s.pose, s.vel, s.row_mask = traj.data_ptr(), pose.data_ptr(), vel.data_ptr(), mask.data_ptr()
    return s


def _table(nets, values):
    from emloco_amd.predictor import ops
    t = ops.LocoValNets(n_nets=len(nets))
    for k, net in enumerate(nets):
        t.net[k] = ops.LocoValNet(net.variant, 0, *[w.data_ptr() for w in _weights(net)], values[k].data_ptr())
    return t


def _single_forward(net, traj, pose, vel, mask, value):
    """the network's own forward-rows, as LocoValEvaluator._forward calls it"""
    from emloco_amd.predictor import ops
    lib, B = ops._lib(), traj.shape[0]
    n_in, h1, h2, _ = DIMS[net.variant]
    f = lambda *s: torch.zeros(*s, device=DEV)
    x, a1, a2, ang = f(B, n_in), f(B, h1), f(B, h2), f(B)
    head = [B, P(traj), 3, P(pose), P(vel), *[P(w) for w in _weights(net)], P(value), P(x), P(a1), P(a2), P(ang)]
    if net.variant == 3:
        ops._chk(lib.emloco_locoval_fwd_rows(*head, P(mask), None), "emloco_locoval_fwd_rows")
    else:
        ops._chk(lib.emloco_locoval_variant_fwd_rows(net.variant, *head, None, P(mask), None), "emloco_locoval_variant_fwd_rows")


# ------------------------------------------------------------------------------------------------ (a) the raw ABI
def test_fwd_multi_equals_each_networks_own_forward_bit_for_bit():
    from emloco_amd.predictor import ops
    B = 37                                                  # no multiple of 4 (rows of a wave) or 16 (rows of a narrow workgroup)
    traj, pose, vel = _inputs(B, seed=23)
    mask = torch.ones(B)
    mask[[0, 5, 6, 18, 30, 36]] = 0
    mask[8:12] = 0                                          # a whole group of four
    mask[16:20] = 0
    mask = mask.to(DEV)
    # all four variants, and two of them a second time with other weights
    nets = [_net(name, DEV, seed=40 + i) for i, name in enumerate(("full", "pose", "vel", "traj", "vel", "full"))]
    assert [n.variant for n in nets] == [3, 2, 1, 0, 1, 3] and not torch.equal(nets[2]._network.fc1.weight, nets[4]._network.fc1.weight)
    keep = {k: t.clone() for k, t in (("traj", traj), ("pose", pose), ("vel", vel), ("mask", mask))}
    values = torch.full((len(nets), B), -7.0, device=DEV)
    s, t = _state(B, traj, pose, vel, mask), _table(nets, values)
    ops._chk(ops._lib().emloco_locoval_eval_fwd_multi(C.byref(s), C.byref(t), None), "emloco_locoval_eval_fwd_multi")
    torch.cuda.synchronize()
    on = mask != 0
    for k, net in enumerate(nets):
        want = torch.full((B,), -7.0, device=DEV)
        _single_forward(net, traj, pose, vel, mask, want)
        torch.cuda.synchronize()
        assert torch.equal(values[k].view(torch.int32), want.view(torch.int32)), (k, net.variant, float((values[k] - want).abs().max()))
        assert bool((values[k][~on] == -7.0).all()) and bool(((values[k][on] > 0) & (values[k][on] < 1)).all())
    assert not torch.equal(values[2][on], values[4][on]) and not torch.equal(values[0][on], values[5][on])
    for k, tns in (("traj", traj), ("pose", pose), ("vel", vel), ("mask", mask)):          # the staged inputs are left as they were
        assert torch.equal(tns, keep[k]), k


# ------------------------------------------------------------------------------------------------ (b) against float64
@pytest.fixture(scope="module")
def float64_errors(B=4096, seed=17):
    """Value error against float64 torch, relative to the largest float64 value, of (`multi`) the new forward's plane of each of the four
    networks and (`full`) the full network's existing kernels on the same inputs and the same function (the network embedded in a
    full one) -- inputs, networks and measure of tests/test_gpu_locoval_variants.py:_float64_errors, every row masked in."""
    from emloco_amd.predictor import ops
    traj, pose, vel = _inputs(B, seed)
    nets = [_net(name, DEV, seed=seed + v, inplace_pose=False) for name, v in VARIANTS.items()]
    values = torch.zeros(len(nets), B, device=DEV)
    mask = torch.ones(B, device=DEV)
    s, t = _state(B, traj, pose, vel, mask), _table(nets, values)
    ops._chk(ops._lib().emloco_locoval_eval_fwd_multi(C.byref(s), C.byref(t), None), "emloco_locoval_eval_fwd_multi")
    torch.cuda.synchronize()
    out = {}
    rel = lambda a, b: float((a.double() - b).abs().max() / b.abs().max())
    for k, (name, v) in enumerate(VARIANTS.items()):
        ref = TorchVariantNet(v).double().to(DEV)
        ref.load_state_dict({kk: p.detach().double() for kk, p in nets[k].state_dict().items()})
        with torch.no_grad():
            v64 = ref(traj.double(), pose.double(), vel.double()).reshape(-1)
            full = nets[k] if v == 3 else _embed_in_full(nets[k], DEV)[0]
            vfull = full(traj.clone(), pose.clone(), vel.clone()).reshape(-1)
        out[name] = {"multi": rel(values[k], v64), "full": rel(vfull, v64)}
    return out


def test_value_planes_against_float64_at_the_variants_tests_bar(float64_errors):
    """The bar of tests/test_gpu_locoval_variants.py::test_variant_kernels_against_float64_within_twice_the_full_kernels_error: the full
    kernels' own error on the same inputs and function is below 1e-4, and a network's error stays within twice it."""
    print("float64 errors:", json.dumps(float64_errors))
    for name, e in float64_errors.items():
        assert 0 < e["full"] < 1e-4, (name, e)
        assert e["multi"] <= 2.0 * e["full"], (name, e)


# ------------------------------------------------------------------------------------------------ (c) end to end
def _run(args, tmp_path, tag):
    out, recs = str(tmp_path / f"{tag}.json"), str(tmp_path / f"{tag}.npz")
    p = subprocess.run([sys.executable, "-m", "emloco_amd.run", "--test", "--num_envs", "64", "--seed", "1", *ENV_ARGS, "--policy_random_init",
                        "--games_num", "32", "--eval_out", out, "--eval_records", recs, *args],
                       cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return json.load(open(out)), dict(np.load(recs)), p.stdout


def test_one_run_with_three_checkpoints_reproduces_three_single_runs(tmp_path):
    names = ("full", "vel", "traj")
    paths = []
    for i, name in enumerate(names):
        paths.append(str(tmp_path / f"{name}.pth"))
        torch.save({k: p.cpu() for k, p in _net(name, "cpu", seed=11 + i).state_dict().items()}, paths[-1])
    rep, rec, stdout = _run(["--valuenet_path", paths[0], "--compare_valuenet", paths[1], "--compare_valuenet", paths[2]], tmp_path, "multi")
    assert set(rep) == {"networks", "paired"} and [n["path"] for n in rep["networks"]] == paths
    assert [n["variant"] for n in rep["networks"]] == [VARIANTS[n] for n in names]
    shared = [k for k in rec if not k.startswith(("value_", "sq_err_"))]
    assert sorted(k for k in rec if k not in shared) == sorted(f"{c}_{i}" for c in ("value", "sq_err") for i in range(3))
    games = rep["paired"]["games"]
    assert games == len(rec["env"]) and games >= 32 and len(rep["paired"]["pairs"]) == 3
    for i, path in enumerate(paths):
        one, one_rec, _ = _run(["--valuenet_path", path], tmp_path, names[i])
        got = rep["networks"][i]["report"]
        for k in one:                                       # the whole report (numbers, moments, printed lines) but the wall clock
            if k != "seconds":
                assert json.dumps(got[k]) == json.dumps(one[k]), (names[i], k, got[k], one[k])
        assert set(one) == set(got)
        assert one_rec["value"].tobytes() == rec[f"value_{i}"].tobytes() and one_rec["sq_err"].tobytes() == rec[f"sq_err_{i}"].tobytes(), names[i]
        for k in shared:                                    # the same games: every shared column of the single run is the multi run's
            assert one_rec[k].tobytes() == rec[k].tobytes(), (names[i], k)
        for ln in one["lines"]:
            assert ln in stdout
    mse = [float(np.mean(rec[f"sq_err_{i}"].astype(np.float64))) for i in range(3)]
    for pr in rep["paired"]["pairs"]:
        assert pr["d_mse"] == mse[pr["b"]] - mse[pr["a"]]


# ------------------------------------------------------------------------------------------------ (d) time
def _time_step(rounds=60, warmup=8, E=4096, period=32):
    """The LocoVal part of a step for the four networks at 4096 envs: `multi` = emloco_locoval_eval_step + _fwd_multi + _finish_multi on
    one state; `passes` = four times (emloco_locoval_eval_step + the network's forward-rows + emloco_locoval_eval_finish), each pass on a
    state of its own -- what four `run.py --test` runs launch per step.  Scripted streams on the device; env e's game ends at step t
    where (t + e) % period == 0, so every step E / period games end and as many start (the first step starts all of them).  The two
    are alternated round by round in one process; median of `rounds` HIP-event timings each, in microseconds."""
    from emloco_amd.learning.locoval_eval import RECORD_WORDS
    from emloco_amd.predictor import ops
    lib, dev = ops._lib(), torch.device(DEV)
    T = warmup + rounds
    G = T // period + 2
    g = torch.Generator().manual_seed(3)
    wp = torch.cumsum(torch.randn(E, 15, 3, generator=g) * 0.3 + 0.2, dim=1).to(dev)
    ip, iv = (torch.randn(E, 24, 3, generator=g) * 0.3).to(dev), torch.randn(E, 2, generator=g).to(dev)
    rr, disc = torch.rand(E, 2, generator=g).to(dev), torch.rand(E, generator=g).to(dev)
    dones = (((torch.arange(T)[:, None] + torch.arange(E)[None, :]) % period) == 0).to(torch.int64).to(dev)
    nets = [_net(name, dev, seed=5 + v) for name, v in VARIANTS.items()]

    def state():
        return eval_state(E, G, 5, 0.99, device=dev, waypoint_traj=wp, init_pose=ip, init_vel=iv)

    N = len(nets)
    ms, mb = state()
    m_values = torch.zeros(N, E, device=dev)
    m_records = torch.zeros(N * E * G * RECORD_WORDS, dtype=torch.int32, device=dev)
    table = _table(nets, m_values)
    singles = []
    for net in nets:
        s, b = state()
        n_in, h1, h2, _ = DIMS[net.variant]
        f = lambda *sh: torch.zeros(*sh, device=dev)
        singles.append(dict(s=s, b=b, value=f(E), scratch=[f(E, n_in), f(E, h1), f(E, h2), f(E)], w=_weights(net), v=net.variant,
                            records=torch.zeros(E * G * RECORD_WORDS, dtype=torch.int32, device=dev)))

    def multi(t):
        ops._chk(lib.emloco_locoval_eval_step(C.byref(ms), P(rr), P(disc), P(dones[t]), None, None, None), "step")
        ops._chk(lib.emloco_locoval_eval_fwd_multi(C.byref(ms), C.byref(table), None), "fwd_multi")
        ops._chk(lib.emloco_locoval_eval_finish_multi(C.byref(ms), C.byref(table), P(m_records), None), "finish_multi")

    def passes(t):
        for q in singles:
            b = q["b"]
            ops._chk(lib.emloco_locoval_eval_step(C.byref(q["s"]), P(rr), P(disc), P(dones[t]), None, None, None), "step")
            head = [E, P(b["traj13"]), 3, P(b["pose"]), P(b["vel"]), *[P(w) for w in q["w"]], P(q["value"]), *[P(x) for x in q["scratch"]]]
            if q["v"] == 3:
                ops._chk(lib.emloco_locoval_fwd_rows(*head, P(b["row_mask"]), None), "fwd_rows")
            else:
                ops._chk(lib.emloco_locoval_variant_fwd_rows(q["v"], *head, None, P(b["row_mask"]), None), "variant_fwd_rows")
            ops._chk(lib.emloco_locoval_eval_finish(C.byref(q["s"]), P(q["value"]), P(q["records"]), None), "finish")

    times = {"multi": [], "passes": []}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(torch.cuda.default_stream(dev)):
        for t in range(T):
            for name, run in (("multi", multi), ("passes", passes)):
                e0.record()
                run(t)
                e1.record()
                e1.synchronize()
                if t >= warmup:
                    times[name].append(e0.elapsed_time(e1) * 1e3)
    torch.cuda.synchronize()
    # what was timed is the comparison the feature promises: the same records, network by network
    for k, q in enumerate(singles):
        assert torch.equal(m_records.view(N, -1)[k], q["records"]), k
        assert torch.equal(mb["games"], q["b"]["games"])
    assert int(mb["games"].sum()) > E
    med = {k: float(np.median(v)) for k, v in times.items()}
    spread = {k: (float(np.min(v)), float(np.max(v))) for k, v in times.items()}
    return med, spread, dict(E=E, period=period, rounds=rounds, warmup=warmup, first_steps=E // period)


def test_the_multi_step_is_not_slower_than_the_four_passes_it_replaces(float64_errors, tmp_path):
    med, spread, cfg = _time_step()
    lines = [f"LocoVal part of an evaluation step for four networks (full / pose / vel / traj) at {cfg['E']} envs, {cfg['first_steps']} games ending and",
             f"starting per step; HIP events around the launches of one step, {cfg['warmup']} warm-up rounds, median of {cfg['rounds']} (min .. max), the two",
             "paths alternated in one process.  multi: eval_step + eval_fwd_multi + eval_finish_multi (3 launches).  passes: four times",
             "eval_step + the network's forward-rows + eval_finish (12 launches), what four single-network runs launch per step.",
             "path      launches    median us   (min .. max)"]
    for name, n in (("multi", 3), ("passes", 12)):
        lines.append(f"{name:8s} {n:9d} {med[name]:12.1f}   ({spread[name][0]:.1f} .. {spread[name][1]:.1f})")
    lines += ["value against float64 torch at B = 4096, every row (largest |kernel - float64| over largest |float64|); in brackets the full",
              "network's existing kernels on the same inputs and the same function:"]
    for name, e in float64_errors.items():
        lines.append(f"{name:8s} {e['multi']:.2e} [{e['full']:.2e}]")
    text = "\n".join(lines) + "\n"
    print(text)
    out = os.environ.get("EMLOCO_LOCOVAL_EVAL_MULTI_TABLE") or str(tmp_path / "locoval_eval_multi.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(text)
    assert med["multi"] <= med["passes"], (med, spread)
