"""Multi-process CPU tests: launcher, native store, host ring, DDP, reference parity."""
import os
import subprocess
import sys

import pytest
import torch

import _workers
from pytorchdistributed_amd.launch import ProcessRaisedException, spawn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("world", [2, 3])
def test_collectives_ring_and_gloo(tmp_path, world):
    spawn(_workers.collectives, args=(world, str(tmp_path)), nprocs=world, timeout=120)
    tot = world * (world + 1) / 2
    for r in range(world):
        d = torch.load(tmp_path / f"{r}.pt", weights_only=True)
        assert torch.allclose(d["t"], torch.full((5,), tot))
        assert torch.allclose(d["r"], torch.arange(11, dtype=torch.float32) * tot)
        assert torch.allclose(d["b"], torch.full((3,), 1.0))
        assert torch.allclose(d["g"], torch.tensor([[q, q * 10.0] for q in range(world)]).flatten())


@pytest.mark.parametrize("backend,abort_first", [("gloo", False), ("ring", False), ("gloo", True)])
def test_ddp_matches_single_process(tmp_path, backend, abort_first):
    """abort_first: a backward that raised halfway (buckets already launched) precedes training."""
    world, steps = 2, 3
    spawn(_workers.ddp_mlp, args=(world, backend, str(tmp_path), steps, abort_first), nprocs=world, timeout=120)
    s0 = torch.load(tmp_path / "0.pt", weights_only=True)
    s1 = torch.load(tmp_path / "1.pt", weights_only=True)
    meta = torch.load(tmp_path / "meta0.pt", weights_only=True)
    assert meta["nb"] > 1  # small caps -> several buckets exercised
    # single-process full-batch reference from rank 0's initial weights
    import torch.nn.functional as F
    from pytorchdistributed_amd.models.mlp import MnistMLP

    torch.manual_seed(123)
    ref = MnistMLP((16, 32, 24, 10))
    opt = torch.optim.SGD(ref.parameters(), lr=0.1, momentum=0.9)
    g = torch.Generator().manual_seed(7)
    X = torch.randn(steps, world * 4, 16, generator=g)
    Y = torch.randint(0, 10, (steps, world * 4), generator=g)
    for s in range(steps):
        opt.zero_grad()
        F.cross_entropy(ref(X[s]), Y[s]).backward()
        opt.step()
    for k, v in ref.state_dict().items():
        assert torch.allclose(s0[k], v, atol=1e-5), k
        assert torch.equal(s0[k], s1[k]), k


def test_reference_ddp_demo_parity(tmp_path):
    """Reference W2 (`ddp_gpus.py`): 2048 samples, bs 32, W=2 -> `Steps: 32`; C=1 soft-target CE -> loss 0."""
    spawn(_workers.reference_ddp_demo, args=(2, 2, 32, str(tmp_path)), nprocs=2, timeout=120)
    for r in range(2):
        log = (tmp_path / f"{r}.log").read_text().strip().splitlines()
        assert log == [f"[GPU: {r}] Epoch: {e} | Batchsize: 32 | Steps: 32" for e in range(2)]
        d = torch.load(tmp_path / f"{r}.pt", weights_only=True)
        assert d["loss"].abs().item() == 0.0


def test_ddp_rejects_mismatched_models(tmp_path):
    """DDP's construction-time cross-rank model check (torch semantics behind `ddp_gpus.py:35`)."""
    spawn(_workers.ddp_mismatch_worker, args=(2, str(tmp_path)), nprocs=2, timeout=120)
    assert (tmp_path / "ok0").exists() and (tmp_path / "ok1").exists()


def test_spawn_propagates_child_exception():
    with pytest.raises(ProcessRaisedException) as ei:
        spawn(_workers.failing_worker, args=(2,), nprocs=2, timeout=60)
    assert "boom from rank 1" in str(ei.value)


def _run(args, env=None, timeout=120):
    e = dict(os.environ)
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    if env:
        e.update(env)
    return subprocess.run([sys.executable, "-m", "pytorchdistributed_amd.run"] + args, cwd=ROOT, env=e,
                          capture_output=True, text=True, timeout=timeout)


def test_pda_run_env_contract(tmp_path):
    script = tmp_path / "w.py"
    script.write_text(
        "import os, json\n"
        "keys=['RANK','LOCAL_RANK','WORLD_SIZE','LOCAL_WORLD_SIZE','MASTER_ADDR','MASTER_PORT','GROUP_RANK']\n"
        f"open(os.path.join({str(tmp_path)!r}, 'env'+os.environ['RANK']), 'w').write(json.dumps({{k: os.environ[k] for k in keys}}))\n")
    r = _run(["--standalone", "--nproc-per-node", "3", str(script)])
    assert r.returncode == 0, r.stderr
    import json

    envs = [json.loads((tmp_path / f"env{i}").read_text()) for i in range(3)]
    assert [e["LOCAL_RANK"] for e in envs] == ["0", "1", "2"]
    assert all(e["WORLD_SIZE"] == "3" and e["LOCAL_WORLD_SIZE"] == "3" for e in envs)


def test_pda_run_tears_down_on_failure(tmp_path):
    script = tmp_path / "w.py"
    script.write_text("import os, time, sys\nif os.environ['RANK']=='1': sys.exit(3)\ntime.sleep(60)\n")
    r = _run(["--standalone", "--nproc-per-node", "2", "--grace", "2", str(script)], timeout=40)
    assert r.returncode == 3


def test_pda_run_simulated_two_nodes_ddp(tmp_path):
    """--nnodes=2 simulated on one host: 2 launchers x 2 workers, DDP all-reduce over gloo."""
    script = tmp_path / "w.py"
    script.write_text(
        "import os, torch\n"
        "import pytorchdistributed_amd.distributed as pd\n"
        "pd.init_process_group('gloo')\n"
        "t = torch.ones(3) * (pd.get_rank() + 1)\n"
        "pd.all_reduce(t)\n"
        f"open(os.path.join({str(tmp_path)!r}, 'o'+str(pd.get_rank())), 'w').write(str(t[0].item()))\n"
        "pd.destroy_process_group()\n")
    from pytorchdistributed_amd.distributed import free_port

    port = str(free_port())
    common = ["--nnodes", "2", "--nproc-per-node", "2", "--master-port", port]
    e = dict(os.environ)
    e["PYTHONPATH"] = ROOT
    p1 = subprocess.Popen([sys.executable, "-m", "pytorchdistributed_amd.run"] + common + ["--node-rank", "1", str(script)],
                          cwd=ROOT, env=e)
    r0 = _run(common + ["--node-rank", "0", str(script)], timeout=120)
    assert p1.wait(timeout=120) == 0
    assert r0.returncode == 0, r0.stderr
    assert [float((tmp_path / f"o{i}").read_text()) for i in range(4)] == [10.0] * 4


def test_pda_run_max_restarts_resumes_from_snapshot(tmp_path):
    """Crash injected at step 5 on rank 1; the launcher restarts the group and training resumes."""
    snap = tmp_path / "snap.pt"
    script = tmp_path / "train.py"
    script.write_text(
        "import os, torch, torch.nn.functional as F\n"
        "from torch.utils.data import DataLoader\n"
        "import pytorchdistributed_amd.distributed as pd\n"
        "from pytorchdistributed_amd.data import DistributedSampler, MyTrainDataset\n"
        "from pytorchdistributed_amd.train import Trainer\n"
        "from pytorchdistributed_amd.models.mlp import linear_20_1\n"
        "pd.init_process_group('gloo')\n"
        "ds = MyTrainDataset(256)\n"
        "dl = DataLoader(ds, batch_size=32, sampler=DistributedSampler(ds))\n"
        "m = linear_20_1()\n"
        "opt = torch.optim.SGD(m.parameters(), lr=1e-3)\n"
        f"tr = Trainer(m, dl, opt, gpu_id=pd.get_rank(), save_every=1, snapshot_path={str(snap)!r}, loss_fn=F.mse_loss)\n"
        "tr.train(3)\n"
        f"open({str(tmp_path / 'done')!r} + os.environ['RANK'], 'w').write(os.environ['PDA_RESTART_COUNT'] + ' ' + str(tr.epochs_run))\n"
        "pd.destroy_process_group()\n")
    r = _run(["--standalone", "--nproc-per-node", "2", "--max-restarts", "1", "--grace", "2", str(script)],
             env={"PDA_FAULT": "1:5:crash"}, timeout=180)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Resuming training from snapshot at Epoch 1" in r.stdout
    assert (tmp_path / "done0").read_text() == "1 1"


@pytest.mark.parametrize("mode", ["size", "op", "missing"])
def test_debug_collectives_checker(tmp_path, mode):
    import json

    spawn(_workers.debug_checker_worker, args=(2, mode, str(tmp_path)), nprocs=2, timeout=120)
    res = [json.loads((tmp_path / f"{r}.json").read_text()) for r in range(2)]
    assert all(r["enabled"] and r["ok_checked"] == 2 for r in res)
    if mode == "missing":
        assert "rank 1 did not reach collective #3" in res[0]["error"]
        return
    for r in res:
        assert r["error"] and "collective mismatch at #3" in r["error"]
        assert "rank 0: all_reduce" in r["error"]
        assert ("[5]" in r["error"]) if mode == "size" else ("rank 1: broadcast" in r["error"])


def test_watchdog_aborts_hung_rank(tmp_path):
    code = ("import time; from pytorchdistributed_amd.utils import watchdog as w; import os;"
            "os.environ['PDA_COLLECTIVE_TIMEOUT_S']='0.3';"
            "from pytorchdistributed_amd.config import set_config; set_config(None);"
            "w.arm('all_reduce bucket 3 (32 MB)'); time.sleep(30)")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert p.returncode != 0
    assert "[pda watchdog] rank 0" in p.stderr and "all_reduce bucket 3 (32 MB)" in p.stderr
    assert "time.sleep" in p.stderr or "File" in p.stderr  # faulthandler stack dump of the hung thread


def test_watchdog_report_mode():
    import time

    from pytorchdistributed_amd import _native

    wd = _native.C().Watchdog(0.2, 0, "report", 17, 0.05)
    t = wd.arm("bucket 0")
    ok = wd.arm("quick", 10.0)
    assert wd.disarm(ok)
    time.sleep(0.5)
    assert wd.expired() == ["bucket 0"] and len(wd.pending()) == 1
    assert wd.disarm(t) and wd.pending() == []
    wd.stop()


def _bench(args, env=None, timeout=240):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR"):
        e.pop(k, None)
    e["PDA_DIST_BACKEND"] = "gloo"
    if env:
        e.update(env)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=e,
                          capture_output=True, text=True, timeout=timeout)


def test_bench_launches_its_own_ranks():
    """`bench.py --gpus 2` without a launcher starts 2 ranks itself (reference `ddp_gpus.py:94-98`
    mp.spawn) and reports the live group's size."""
    import json

    r = _bench(["--gpus", "2", "--steps", "1", "--warmup", "1"])
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout  # rank 0 only
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["config"]["parallelism"] == "dp2"
    assert rec["backend"] == "gloo" and rec["config"]["global_batch"] == 2 * rec["config"]["per_gpu_batch"]


def test_bench_dump_outputs_repeatable(tmp_path, monkeypatch):
    """`--dump-outputs DIR` writes the last timed step's loss, logits and parameter sample as float32
    .npy files; the seeded run repeats them exactly; `--steps` is the number of timed steps and the line
    carries `ms_per_step`; `--full` is accepted.  A second value of `--steps` runs that many."""
    import json

    import numpy as np

    monkeypatch.delenv("PDA_DETERMINISTIC", raising=False)
    got = []
    for d, extra in ((tmp_path / "a", []), (tmp_path / "b", ["--full"])):
        r = _bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(d)] + extra)
        assert r.returncode == 0, r.stderr[-3000:]
        rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        # the step count is counted by the run (losses recorded after the warm-up), not echoed
        assert rec["steps"] == 2 and rec["timed_steps_run"] == 2 and rec["ms_per_step"] > 0
        assert rec["fixed_order_sums"] is True  # a dumping run asks for the fixed-order sums
        assert sorted(p.name for p in d.iterdir()) == ["logits.npy", "loss.npy", "params_sample.npy"]
        arrs = {p.stem: np.load(p) for p in d.iterdir()}
        assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrs.values())
        assert arrs["logits"].shape == (rec["config"]["per_gpu_batch"], 1000) and arrs["loss"].shape == (1,)
        assert abs(float(arrs["loss"][0]) - rec["final_loss"]) < 1e-3
        got.append(arrs)
    for k in got[0]:
        assert np.array_equal(got[0][k], got[1][k]), k
    r = _bench(["--gpus", "1", "--steps", "3", "--warmup", "0"])
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert rec["timed_steps_run"] == 3 and rec["fixed_order_sums"] is False


def test_bench_refuses_mismatched_world():
    """Under a launcher whose WORLD_SIZE disagrees with --gpus the bench refuses (never downgrades)."""
    r = _bench(["--gpus", "2", "--steps", "1", "--warmup", "0"], env={"WORLD_SIZE": "1", "RANK": "0",
                                                                        "LOCAL_RANK": "0"})
    assert r.returncode != 0
    assert "refusing" in r.stderr


def test_bench_rank_failure_fails_the_launch():
    """One rank failing makes the self-launched run exit non-zero (the group is torn down)."""
    r = _bench(["--gpus", "2", "--steps", "1", "--warmup", "0", "--image", "-3"], timeout=120)
    assert r.returncode != 0


def test_ddp_rebuilds_buckets_in_gradient_order(tmp_path):
    """A model whose gradients arrive in a different order than reverse registration: after the first
    backward DDP rebuilds its buckets in the observed order (torch Reducer semantics behind
    `ddp_gpus.py:35`), and training still matches single-process full-batch SGD."""
    world, steps = 2, 3
    spawn(_workers.ddp_rebuild_worker, args=(world, str(tmp_path), steps), nprocs=world, timeout=120)
    d0 = torch.load(tmp_path / "0.pt", weights_only=True)
    d1 = torch.load(tmp_path / "1.pt", weights_only=True)
    assert d0["rebuilt"] and d1["rebuilt"]
    assert d0["after"] == d1["after"] and d0["before"] != d0["after"]
    import torch.nn.functional as F

    torch.manual_seed(5)
    ref = _workers._Swapped()
    opt = torch.optim.SGD(ref.parameters(), lr=0.1)
    g = torch.Generator().manual_seed(9)
    X = torch.randn(steps, world * 4, 16, generator=g)
    Y = torch.randint(0, 10, (steps, world * 4), generator=g)
    for s in range(steps):
        opt.zero_grad()
        F.cross_entropy(ref(X[s]), Y[s]).backward()
        for n, p in ref.named_parameters():  # every step's averaged gradient, before and after the rebuild
            assert torch.allclose(d0["grads"][s][n], p.grad, atol=1e-6), (s, n)
        opt.step()
    for k, v in ref.state_dict().items():
        assert torch.allclose(d0["state"][k], v, atol=1e-5), k
        assert torch.equal(d0["state"][k], d1["state"][k]), k


def test_ddp_fp32_gradient_reduction(tmp_path):
    """PDA_GRAD_REDUCE_DTYPE=fp32 on bf16 parameters: the averaged gradient is the fp32 mean of the
    ranks' bf16 gradients rounded once (no bf16 partial sums)."""
    world = 2
    spawn(_workers.ddp_fp32_reduce_worker, args=(world, str(tmp_path)), nprocs=world, timeout=120)
    d = torch.load(tmp_path / "0.pt", weights_only=True)
    for n, g in d["ddp"].items():
        want = (sum(loc[n].float() for loc in d["local"]) / world).to(torch.bfloat16)
        assert torch.equal(g, want), n


_FAULT_FSDP = r'''
import os, sys, torch, torch.nn.functional as F
sys.path.insert(0, os.path.join({root!r}, "tests"))
import pytorchdistributed_amd.distributed as pd
from pytorchdistributed_amd.parallel.fsdp import FullyShardedDataParallel
from pytorchdistributed_amd.utils.fault import maybe_inject
from _workers import _Net, _Block
pd.init_process_group("gloo")
rank = pd.get_rank()
torch.manual_seed(0)
model = FullyShardedDataParallel(_Net(), unit_types=(_Block,))
opt = torch.optim.SGD(model.parameters(), lr=1e-2)
for step in range(4):
    maybe_inject(rank, step)
    F.cross_entropy(model(torch.randn(4, 8)), torch.randint(0, 4, (4,))).backward()
    opt.step(); opt.zero_grad()
pd.destroy_process_group()
'''

_FAULT_PP = r'''
import os, sys, torch, torch.nn.functional as F
sys.path.insert(0, os.path.join({root!r}, "tests"))
import pytorchdistributed_amd.distributed as pd
from pytorchdistributed_amd.parallel.pipeline import Pipeline
from pytorchdistributed_amd.utils.fault import maybe_inject
from _workers import _tiny_stack
pd.init_process_group("gloo")
rank = pd.get_rank()
full = _tiny_stack(4)
stage = torch.nn.Sequential(*list(full)[6 * rank: 6 * rank + 6])
pipe = Pipeline(stage, [0, 1], num_microbatches=4, schedule="{schedule}", loss_fn=F.mse_loss, device=torch.device("cpu"))
for step in range(4):
    maybe_inject(rank, step)
    pipe.step(torch.randn(8, 16), torch.randn(8, 16))
pd.destroy_process_group()
'''


@pytest.mark.parametrize("kind,schedule", [("fsdp", None), ("pp", "1f1b"), ("pp", "gpipe")])
def test_watchdog_fault_injection_ends_run(tmp_path, kind, schedule):
    """SURVEY §5.3 / VERDICT r4 #2: one rank hangs (PDA_FAULT) at step 1; the peer's FSDP all-gather or
    pipeline P2P wait is under a watchdog ticket, so the job ends non-zero with the pending operation and
    Python stacks printed, well inside the test's timeout — not a silent hang."""
    src = (_FAULT_FSDP if kind == "fsdp" else _FAULT_PP).replace("{root!r}", repr(ROOT)).replace("{schedule}", str(schedule))
    script = tmp_path / "w.py"
    script.write_text(src)
    env = {"PDA_FAULT": "1:1:hang", "PDA_COLLECTIVE_TIMEOUT_S": "4", "PDA_WATCHDOG_ACTION": "abort"}
    r = _run(["--standalone", "--nproc-per-node", "2", "--grace", "2", str(script)], env=env, timeout=150)
    assert r.returncode != 0
    assert "[fault] rank 1 step 1: injecting hang" in r.stderr
    assert "[pda watchdog] rank 0: collective timeout" in r.stderr, r.stderr[-3000:]
    want = "fsdp c10d all_gather" if kind == "fsdp" else "pp "
    assert want in r.stderr, r.stderr[-3000:]
    assert "File " in r.stderr  # faulthandler stack dump


def test_parameter_server_matches_single_process(tmp_path):
    """SURVEY X17 (PS-worker concept, NB02:28-31): reduce-to-server + server-side SGD + broadcast
    equals full-batch single-process SGD; every rank ends with the server's parameters."""
    world, steps = 2, 3
    spawn(_workers.param_server_worker, args=(world, str(tmp_path), steps), nprocs=world, timeout=120)
    import torch.nn.functional as F
    from pytorchdistributed_amd.models.mlp import MnistMLP

    torch.manual_seed(123)
    ref = MnistMLP((16, 32, 24, 10))
    opt = torch.optim.SGD(ref.parameters(), lr=0.1, momentum=0.9)
    g = torch.Generator().manual_seed(7)
    X = torch.randn(steps, world * 4, 16, generator=g)
    Y = torch.randint(0, 10, (steps, world * 4), generator=g)
    for s in range(steps):
        opt.zero_grad()
        F.cross_entropy(ref(X[s]), Y[s]).backward()
        opt.step()
    s0 = torch.load(tmp_path / "0.pt", weights_only=True)
    s1 = torch.load(tmp_path / "1.pt", weights_only=True)
    for k, v in ref.state_dict().items():
        assert torch.allclose(s0[k], v, atol=1e-5), k
        assert torch.equal(s0[k], s1[k]), k


def test_parameter_server_frozen_and_unused_params(tmp_path):
    """Frozen parameters are synced from the server at construction; a parameter without a gradient on
    every rank is not stepped by the server's optimizer (weight decay / momentum would move it)."""
    spawn(_workers.param_server_unused_frozen_worker, args=(2, str(tmp_path)), nprocs=2, timeout=120)
    s0 = torch.load(tmp_path / "0.pt", weights_only=True)
    s1 = torch.load(tmp_path / "1.pt", weights_only=True)
    for k in s0["start"]:
        assert torch.equal(s0["start"][k], s1["start"][k]), k  # every rank starts from the server's state
        assert torch.equal(s0["end"][k], s1["end"][k]), k
    for k in ("unused.weight", "unused.bias", "frozen.weight", "frozen.bias"):
        assert torch.equal(s0["start"][k], s0["end"][k]), k
    assert not torch.equal(s0["start"]["used.weight"], s0["end"]["used.weight"])
