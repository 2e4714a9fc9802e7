"""Single-process CPU unit tests: sampler parity, bucket reducer, native store,
optimizers' reference math, model shapes / parameter counts, log format, checkpoint layout."""
import sys
import threading

import pytest
import torch
import torch.nn.functional as F
from hypothesis import given, settings, strategies as st

from pytorchdistributed_amd import _native
from pytorchdistributed_amd.data import DistributedSampler, MyTrainDataset, SimpleDataset, random_image_batch


class _Len:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


@settings(max_examples=150, deadline=None)
@given(n=st.integers(1, 300), w=st.integers(1, 9), epoch=st.integers(0, 5), shuffle=st.booleans(),
       drop_last=st.booleans(), seed=st.integers(0, 1000))
def test_sampler_matches_torch(n, w, epoch, shuffle, drop_last, seed):
    if drop_last and n < w:
        return
    ds = _Len(n)
    for r in range(w):
        ours = DistributedSampler(ds, num_replicas=w, rank=r, shuffle=shuffle, seed=seed, drop_last=drop_last)
        ref = torch.utils.data.DistributedSampler(ds, num_replicas=w, rank=r, shuffle=shuffle, seed=seed,
                                                  drop_last=drop_last)
        ours.set_epoch(epoch)
        ref.set_epoch(epoch)
        assert list(ours) == list(ref)
        assert len(ours) == len(ref)


def test_sampler_reference_numbers():
    # 2048/2 -> 1024 per rank, disjoint; 10/3 padding wraps -> rank 2 gets 4 items
    s0 = DistributedSampler(_Len(2048), 2, 0)
    s1 = DistributedSampler(_Len(2048), 2, 1)
    assert len(s0) == len(s1) == 1024
    assert not (set(s0) & set(s1))
    assert len(list(DistributedSampler(_Len(10), 3, 2, shuffle=False))) == 4
    assert list(DistributedSampler(_Len(10), 3, 2, shuffle=False)) == [2, 5, 8, 1]


def test_reducer_buckets_and_order():
    C = _native.C()
    numels = [1000, 50, 3000, 7, 2000, 64]
    r = C.BucketReducer(numels, [2] * 6, [1] * 6, 4000, 1000, 8, [])
    seen = []
    for b in range(r.num_buckets):
        ps = r.bucket_params(b)
        seen += ps
        offs = r.bucket_offsets(b)
        assert all(o % 8 == 0 for o in offs)
        assert r.bucket_numel(b) >= sum(numels[p] for p in ps)
    assert sorted(seen) == list(range(6))
    assert seen == [5, 4, 3, 2, 1, 0]  # reverse registration order
    # buckets only launch in index order even if a later bucket is ready first
    r.prepare()
    last_bucket_params = r.bucket_params(r.num_buckets - 1)
    launched = []
    for p in last_bucket_params:
        launched += r.mark_ready(p)
    assert launched == [] or launched == [0]
    for p in range(6):
        if p not in last_bucket_params:
            launched += r.mark_ready(p)
    assert launched == list(range(r.num_buckets))
    assert r.all_launched()
    with pytest.raises(RuntimeError):
        r.mark_ready(0)


def test_reducer_dtype_split_and_flush():
    C = _native.C()
    r = C.BucketReducer([10, 10, 10], [4, 2, 4], [0, 1, 0], 1 << 20, 1 << 20, 8, [])
    assert {r.bucket_dtype(b) for b in range(r.num_buckets)} == {0, 1}
    r.prepare()
    r.mark_ready(0)
    assert sorted(r.unready_params()) == [1, 2]
    assert r.flush_unready() != []
    assert r.all_launched()


def test_native_store_blocking_get_and_ops():
    C = _native.C()
    srv = C.StoreServer("127.0.0.1", 0)
    a = C.StoreClient("127.0.0.1", srv.port, 10.0)
    b = C.StoreClient("127.0.0.1", srv.port, 10.0)
    out = {}
    t = threading.Thread(target=lambda: out.setdefault("v", b.get("late")))
    t.start()
    a.set("late", b"value")
    t.join(5)
    assert out["v"] == b"value"
    assert a.add("ctr", 2) == 2 and b.add("ctr", 3) == 5
    assert a.compare_set("cas", b"", b"x") == b"x"
    assert a.compare_set("cas", b"nope", b"y") == b"x"
    assert a.check(["late", "ctr"]) and not a.check(["missing"])
    assert a.delete_key("late") and not a.check(["late"])
    with pytest.raises(Exception):
        c = C.StoreClient("127.0.0.1", srv.port, 0.3)
        c.get("never")
    srv.stop()


def test_fused_optim_cpu_reference_math():
    from pytorchdistributed_amd.optim import SGD, Adam, AdamW

    for ours_cls, ref_cls, kw in [(SGD, torch.optim.SGD, dict(lr=0.1, momentum=0.9, weight_decay=1e-3, nesterov=True)),
                                  (Adam, torch.optim.Adam, dict(lr=1e-2, weight_decay=1e-2)),
                                  (AdamW, torch.optim.AdamW, dict(lr=1e-2, weight_decay=1e-2))]:
        torch.manual_seed(0)
        p1 = torch.nn.Parameter(torch.randn(37))
        p2 = torch.nn.Parameter(p1.detach().clone())
        o1, o2 = ours_cls([p1], **kw), ref_cls([p2], **kw)
        for _ in range(4):
            g = torch.randn(37)
            p1.grad, p2.grad = g.clone(), g.clone()
            o1.step()
            o2.step()
        assert torch.allclose(p1, p2, atol=1e-6), ours_cls


def test_models_param_counts_and_shapes():
    from pytorchdistributed_amd.models import TutorialMLP, resnet50, linear_20_1
    from pytorchdistributed_amd.models.resnet import from_torchvision_state_dict, to_torchvision_state_dict

    m = resnet50()
    assert sum(p.numel() for p in m.parameters()) == 25_557_032  # `03_model_parallel.ipynb` raw line 301
    assert sum(p.numel() for p in TutorialMLP().parameters()) == 1165
    assert sum(p.numel() for p in linear_20_1().parameters()) == 21
    y = m(torch.randn(2, 3, 64, 64))  # NCHW input accepted
    assert y.shape == (2, 1000)
    sd = to_torchvision_state_dict(m)
    assert sd["conv1.weight"].shape == (64, 3, 7, 7) and sd["layer1.0.conv2.weight"].shape == (64, 64, 3, 3)
    m2 = resnet50()
    from_torchvision_state_dict(m2, sd)
    assert torch.equal(m2.layer3[2].conv2.weight, m.layer3[2].conv2.weight)


def test_reference_datasets():
    ds = MyTrainDataset(2048)
    x, y = ds[0]
    assert x.shape == (20,) and y.shape == (1,)
    assert torch.equal(MyTrainDataset(16)[3][0], MyTrainDataset(16)[3][0])  # seeded: same on every rank
    s = SimpleDataset(1000)
    assert s[0][0].shape == (10,) and s.labels.unique().tolist() == [0]
    xb, yb = random_image_batch(120, (128, 128), 1000)
    assert xb.shape == (120, 3, 128, 128) and torch.equal(yb.sum(1), torch.ones(120))


def test_reference_quirk_ce_c1_is_zero():
    # soft-target CE with one logit -> loss 0, grad 0
    from pytorchdistributed_amd.ops import cross_entropy

    out = torch.randn(32, 1, requires_grad=True)
    loss = cross_entropy(out, torch.rand(32, 1))
    loss.backward()
    assert loss.abs().item() == 0.0 and out.grad.abs().sum().item() == 0.0


def test_epoch_log_line():
    from pytorchdistributed_amd.utils.log import epoch_line

    assert epoch_line(1, 4, 32, 32) == "[GPU: 1] Epoch: 4 | Batchsize: 32 | Steps: 32"


def test_checkpoint_layout_loads_with_plain_torch(tmp_path):
    from pytorchdistributed_amd.models import TutorialMLP
    from pytorchdistributed_amd.utils.checkpoint import load_snapshot, save_snapshot

    m = TutorialMLP()
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    path = str(tmp_path / "snap.pt")
    save_snapshot(path, m, opt, epochs_run=3)
    snap = torch.load(path, weights_only=True)
    assert set(snap) >= {"MODEL_STATE", "OPTIMIZER_STATE", "EPOCHS_RUN", "RNG"}
    assert not any(k.startswith("module.") for k in snap["MODEL_STATE"])
    m2 = TutorialMLP()
    assert load_snapshot(path, m2, torch.optim.SGD(m2.parameters(), lr=0.1)) == 3
    assert torch.equal(m2.fc1.weight, m.fc1.weight)


def test_cpu_ops_match_torch():
    from pytorchdistributed_amd import ops

    x = torch.randn(2, 9, 9, 16)
    w = torch.randn(8, 3, 3, 16)
    y = ops.conv2d(x, w, stride=2, padding=1)
    ref = F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), None, 2, 1).permute(0, 2, 3, 1)
    assert torch.allclose(y, ref, atol=1e-5)
    p = ops.max_pool2d(x)
    assert p.shape == (2, 5, 5, 16)
    assert torch.allclose(ops.global_avg_pool2d(x), x.mean((1, 2)))


def test_transformer_models_cpu():
    from pytorchdistributed_amd.models.gpt2 import GPT2, GPT2Stage, config as gcfg
    from pytorchdistributed_amd.models.llama import Llama, config as lcfg

    g = GPT2(gcfg("gpt2", n_layer=2, n_embd=64, n_head=2, n_positions=32, vocab_size=100))
    idx = torch.randint(0, 100, (2, 32))
    loss = g(idx, idx)
    loss.backward()
    assert g.cfg.padded_vocab == 128 and g.wte.grad[100:].abs().sum() == 0  # padded rows get no gradient
    assert torch.isfinite(loss)
    full = gcfg("gpt2-medium")
    assert GPT2(gcfg("gpt2", n_layer=1, n_embd=64, n_head=2), device="meta").num_params() > 0
    # GPT-2 medium / XL and Llama-3-8B parameter counts (standard architectures)
    gm = GPT2(full, device="meta")
    assert abs(gm.num_params() - 354.8e6) / 354.8e6 < 0.01
    gx = GPT2(gcfg("gpt2-xl"), device="meta")
    assert abs(gx.num_params() - 1.558e9) / 1.558e9 < 0.01
    lm = Llama(lcfg("llama3-8b"), device="meta")
    assert abs(sum(p.numel() for p in lm.parameters()) - 8.03e9) / 8.03e9 < 0.01
    tl = Llama(lcfg("llama3-tiny", dim=64, n_heads=2, n_kv_heads=1, ffn_dim=128))
    out = tl(torch.randint(0, 1024, (2, 16)), torch.randint(0, 1024, (2, 16)))
    out.backward()
    st = GPT2Stage(gcfg("gpt2", n_layer=4, n_embd=64, n_head=2, vocab_size=100), 0, 2, True, False)
    assert st(idx).shape == (2, 32, 64)


def test_grad_join_sums_consumers_without_autograd_add():
    from pytorchdistributed_amd.ops.grad_join import GradJoin

    class Scale(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, k, join):
            ctx.k, ctx.join = k, join
            return x * k

        @staticmethod
        def backward(ctx, g):
            return ctx.join.contribute(g * ctx.k), None, None

    for consumers in (2, 3):
        x = torch.randn(5, requires_grad=True)
        j = GradJoin(consumers)
        ks = [2.0, -3.0, 0.5][:consumers]
        sum(Scale.apply(x, k, j) for k in ks).sum().backward()
        assert torch.allclose(x.grad, torch.full((5,), sum(ks)))
        assert j.pending is None and j.arrived == 0


def test_optimizer_device_step_counter_bookkeeping():
    """`_device_step` advances once per step() call, tracks the host counter, refuses a parameter
    whose host step diverged, and `advance_steps` accounts for graph replays."""
    from pytorchdistributed_amd.optim import Adam

    p = torch.nn.Parameter(torch.zeros(4))
    opt = Adam([p])
    dev = torch.device("cpu")
    opt._step_calls = 1
    t = opt._device_step(dev, 1)
    assert t is not None and t.item() == 1.0
    assert opt._device_step(dev, 1) is t and t.item() == 1.0  # same step() call: no second increment
    assert opt._device_step(dev, 3) is None                    # diverged host step: host path
    opt._step_calls = 2
    assert opt._device_step(dev, 2).item() == 2.0
    opt.state[p]["step"] = 2
    opt.advance_steps(5)
    assert opt.state[p]["step"] == 7 and opt._dstep[dev][0] == 7


def test_grad_join_masked_grad():
    """A MaskedGrad stashed in a GradJoin (bottleneck residual gradient dz * relu_mask, kept as dz + bits)
    materialises to the dense masked gradient on every generic path."""
    from pytorchdistributed_amd.ops.grad_join import GradJoin, MaskedGrad

    torch.manual_seed(0)
    dz = torch.randn(2, 3, 4, 8)
    mask = torch.rand(2, 3, 4, 8) > 0.5
    bits = (mask.reshape(-1, 8).to(torch.uint8) << torch.arange(8, dtype=torch.uint8)).sum(1).to(torch.uint8)
    mg = MaskedGrad(dz, bits)
    assert torch.equal(mg.materialize(), dz * mask)
    j = GradJoin(2)
    j.stash(mg)
    other = torch.randn_like(dz)
    assert torch.allclose(j.contribute(other), other + dz * mask)
    j3 = GradJoin(3)
    j3.stash(mg)
    j3.stash(other)
    assert torch.allclose(j3.take(), other + dz * mask)


def test_xgmi_tuning_table_from_sweep(tmp_path, monkeypatch):
    """tools/bench_allreduce.py --write-table: per size the fastest transport, equal neighbours merged,
    last range open-ended; load_table checks the world size and the algorithm names."""
    import json

    from pytorchdistributed_amd.parallel import xgmi

    def rec(mb, r, o, t):
        return {"size_mb": mb, "rccl": {"ms": r}, "xgmi_oneshot": {"ms": o}, "xgmi_twoshot": {"ms": t}}

    recs = [rec(0.25, 0.05, 0.01, 0.02), rec(1, 0.06, 0.02, 0.03), rec(4, 0.10, 0.09, 0.05), rec(64, 0.5, 2.0, 0.6)]
    tab = xgmi.table_from_sweep(recs, 8)
    assert tab["world"] == 8
    assert [e["algo"] for e in tab["entries"]] == ["oneshot", "twoshot", "rccl"]
    assert tab["entries"][0]["max_bytes"] == 2 ** 20 and tab["entries"][1]["max_bytes"] == 4 * 2 ** 20
    assert tab["entries"][-1]["max_bytes"] >= 1 << 60
    p = tmp_path / "t.json"
    p.write_text(json.dumps(tab))
    assert xgmi.load_table(8, str(p)) == tab["entries"]
    assert xgmi.load_table(4, str(p)) is None  # table of another world size
    monkeypatch.setenv("PDA_XGMI_TUNING", str(p))
    assert xgmi.load_table(8) == tab["entries"]


def test_side_stream_join_is_per_backward_pass(monkeypatch):
    """ops/streams.py queues one join callback per autograd graph task: a backward that raised (its
    final callbacks never run) must not stop the next backward from queueing its own join."""
    import torch

    from pytorchdistributed_amd.ops import streams

    queued = []
    monkeypatch.setattr(streams, "side_stream", lambda device: None)

    class _Eng:
        @staticmethod
        def queue_callback(cb):
            queued.append(cb)

    monkeypatch.setattr(torch.autograd.Variable, "_execution_engine", _Eng)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda idx=None: None)
    monkeypatch.setattr(torch.cuda, "stream", lambda s: __import__("contextlib").nullcontext())

    class _S:
        def wait_stream(self, other):
            pass

    monkeypatch.setattr(streams, "side_stream", lambda device: _S())
    dev = torch.device("cuda", 0)
    ids = iter([5, 5, 6])
    monkeypatch.setattr(torch._C, "_current_graph_task_id", lambda: next(ids))
    for _ in range(2):  # same graph task: one callback
        with streams.wgrad_stream(dev):
            pass
    assert len(queued) == 1
    with streams.wgrad_stream(dev):  # a new task although the first never joined
        pass
    assert len(queued) == 2
    streams._join_pending.clear()
    streams._join_task.clear()


def test_bn_dual_guard_channel_counts():
    """bn_dual_ok: register-table channel counts only (C = 1536 needs 3 sets per lane -> separate BN),
    and a C < 8 query returns false instead of dividing by zero on the host."""
    C = _native.C

    assert C().bn_dual_ok(2048) and C().bn_dual_ok(256)
    assert not C().bn_dual_ok(1536)
    assert not C().bn_dual_ok(0) and not C().bn_dual_ok(4)


def test_resnet_snapshot_in_torchvision_layout(tmp_path):
    """ResNet-50 snapshots carry MODEL_STATE in the reference's torchvision layout (top-level conv1 / bn1,
    OIHW conv weights; `03_model_parallel.ipynb` raw lines 107-110, 314), so a stock torchvision
    ResNet-50 could load them; load_snapshot converts back to the channels-last model exactly."""
    from pytorchdistributed_amd.models.resnet import resnet50
    from pytorchdistributed_amd.utils.checkpoint import load_snapshot, save_snapshot

    torch.manual_seed(0)
    m = resnet50()
    path = str(tmp_path / "snap.pt")
    save_snapshot(path, m, None, epochs_run=1)
    snap = torch.load(path, weights_only=True)
    sd = snap["MODEL_STATE"]
    assert snap["LAYOUT"] == "reference"
    assert tuple(sd["conv1.weight"].shape) == (64, 3, 7, 7)  # torchvision shapes / names
    assert tuple(sd["layer1.0.conv2.weight"].shape) == (64, 64, 3, 3)
    assert tuple(sd["layer4.2.conv3.weight"].shape) == (2048, 512, 1, 1)
    assert tuple(sd["fc.weight"].shape) == (1000, 2048) and "bn1.running_var" in sd
    assert "layer1.0.downsample.0.weight" in sd and "layer1.0.downsample.1.num_batches_tracked" in sd
    assert not any(k.startswith("stem.") for k in sd) and sum(v.numel() for k, v in sd.items()
                                                             if not k.endswith(("running_mean", "running_var",
                                                                                "num_batches_tracked"))) == 25557032
    m2 = resnet50()
    assert load_snapshot(path, m2) == 1
    for (k, a), (_, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k


def test_data_parallel_coalesced_replicas_match_single_device():
    """DataParallel replicas built from one coalesced copy per dtype (forced copy on the CPU tier):
    outputs and master gradients equal the plain module's; the replica state views one flat copy."""
    import torch.nn as tnn

    from pytorchdistributed_amd.parallel.dp import DataParallel

    torch.manual_seed(0)
    net = tnn.Sequential(tnn.Linear(6, 8), tnn.BatchNorm1d(8), tnn.ReLU(), tnn.Linear(8, 3))
    ref = tnn.Sequential(tnn.Linear(6, 8), tnn.BatchNorm1d(8), tnn.ReLU(), tnn.Linear(8, 3))
    ref.load_state_dict(net.state_dict())
    dp = DataParallel(net, device_ids=["cpu", "cpu"])
    dp._force_copy = True
    st = dp._replica_states([torch.device("cpu"), torch.device("cpu")])
    w0, b0 = st[1]["0.weight"], st[1]["0.bias"]
    assert w0.untyped_storage().data_ptr() == b0.untyped_storage().data_ptr()  # one flat copy
    assert w0.data_ptr() != net[0].weight.data_ptr()
    x = torch.randn(10, 6)
    out = dp(x)
    # reference: the two halves through the module separately (per-replica BN batch statistics)
    ref_out = torch.cat([ref(x[:5]), ref(x[5:])])
    assert torch.allclose(out, ref_out, atol=1e-6)
    out.square().sum().backward()
    ref_out.square().sum().backward()
    for (n, p), (_, q) in zip(net.named_parameters(), ref.named_parameters()):
        assert torch.allclose(p.grad, q.grad, atol=1e-5), n
    # persistent replica: a second forward refreshes the same buffer (one copy per group, no new allocation)
    copies = dp.replica_copies
    st2 = dp._replica_states([torch.device("cpu"), torch.device("cpu")])
    assert st2[1]["0.weight"].data_ptr() == w0.data_ptr()
    assert dp.replica_copies - copies == len(dp._groups)
    # the master's parameters are views of one flat buffer; an optimizer step through them shows in the replica
    with torch.no_grad():
        net[0].weight.add_(1.0)
    st3 = dp._replica_states([torch.device("cpu"), torch.device("cpu")])
    assert torch.equal(st3[1]["0.weight"], net[0].weight)
    # a parameter replaced after wrapping is picked up (re-flattened), not silently dropped
    net[3].weight = tnn.Parameter(torch.zeros(3, 8))
    st4 = dp._replica_states([torch.device("cpu"), torch.device("cpu")])
    assert torch.equal(st4[1]["3.weight"], torch.zeros(3, 8))


def test_data_parallel_threads_leave_the_module_intact():
    """The per-device threads of a DataParallel forward must not swap tensors through one shared module:
    with the interpreter switching threads as often as it can, after every forward + backward the
    wrapped module's parameters are still its own leaf tensors and all have gradients."""
    import torch.nn as tnn

    from pytorchdistributed_amd.parallel.dp import DataParallel

    torch.manual_seed(0)
    net = tnn.Sequential(tnn.Linear(6, 8), tnn.BatchNorm1d(8), tnn.ReLU(), tnn.Linear(8, 3))
    dp = DataParallel(net, device_ids=["cpu", "cpu", "cpu"])
    dp._force_copy = True
    own = [p for p in net.parameters()]
    x = torch.randn(12, 6)
    interval = sys.getswitchinterval()
    sys.setswitchinterval(1e-6)
    try:
        for it in range(100):
            net.zero_grad()
            dp(x).square().sum().backward()
            now = list(net.parameters())
            assert all(a is b for a, b in zip(own, now)), it
            assert all(p.is_leaf and p.grad is not None for p in now), it
    finally:
        sys.setswitchinterval(interval)
