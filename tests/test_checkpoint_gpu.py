"""Checkpoints on the HIP kernels: a program built from a checkpoint file
computes, bit for bit, what the program compiled from the module that wrote the
file computes; top-k through HipExecutor (captured graph, eager, guard rerun)."""
import numpy as np
import pytest
import torch

from idunno.models import HipRunner
from idunno.models import packed as P
from idunno.models import reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASES = [("resnet18", 4), ("resnet50", 4), ("alexnet", 6)]


@pytest.fixture(scope="module")
def ops():
    from idunno import ops as o

    o.load()
    return o


def _runner(prog, dtype):
    r = HipRunner(prog, DEV)
    if dtype == "fp32":
        assert r.split and r._split_ok()
    return r


_SEED0 = {}


def _seed0_logits(ops, name, B, dtype):
    """Logits of the seed-0 program (the parameters every runner had before checkpoints), once per case."""
    key = (name, B, dtype)
    if key not in _SEED0:
        img = ops.synth_images(0, 0, B, DEV)
        _SEED0[key] = _runner(P.build_program(name, seed=0, dtype=dtype), dtype).logits(img).clone()
    return _SEED0[key]


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("name,B", CASES)
def test_checkpoint_program_equals_source_program(ops, tmp_path, name, B, dtype):
    m = ref.build(name, seed=3, randomize_bn=True)
    path = str(tmp_path / f"{name}.pth")
    torch.save(m.state_dict(), path)
    img = ops.synth_images(0, 0, B, DEV)
    want = _runner(P.compile_model(m, name, dtype), dtype).logits(img)
    got = _runner(P.build_program(name, dtype=dtype, weights=path), dtype).logits(img)
    assert got.shape == (B, 1000) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    assert torch.equal(got, want)
    assert not torch.equal(got, _seed0_logits(ops, name, B, dtype))      # the file's parameters, not the seed's


@pytest.mark.parametrize("name,B", CASES)
def test_seed0_checkpoint_meets_the_fp64_oracle_bound(ops, tmp_path, name, B):
    """tests/test_split.py::test_model_split_vs_fp64_oracle's bound (1e-5 of the
    largest logit, same argmax) for the same module, served from a checkpoint."""
    m = ref.build(name, seed=0)
    path = str(tmp_path / f"{name}.safetensors")
    from safetensors.torch import save_file

    save_file({k: v.contiguous() for k, v in m.state_dict().items()}, path)
    img = ops.synth_images(0, 0, B, DEV)
    z = _runner(P.build_program(name, seed=77, dtype="fp32", weights=path), "fp32").logits(img)
    assert torch.equal(z, _seed0_logits(ops, name, B, "fp32"))
    got = z.double().cpu()
    with torch.no_grad():
        want = m.double()(ref.preprocess_u8(img.cpu()).double())
    err = (got - want).abs().max().item() / want.abs().max().item()
    print(f"{name} B={B}: rel logit err vs fp64 {err:.2e}")
    assert err <= 1e-5, f"{name}: rel logit err {err:.2e}"
    assert torch.equal(got.argmax(1), want.argmax(1))


def _stable_ref(z, k):
    z = z.double().cpu()
    idx = torch.sort(z, dim=1, descending=True, stable=True).indices[:, :k]
    return idx, torch.softmax(z, 1).gather(1, idx)


def test_hip_executor_checkpoint_topk_graph_equals_eager(ops, tmp_path):
    from idunno.runtime.executor import HipExecutor

    m = ref.build("resnet18", seed=3, randomize_bn=True)
    path = str(tmp_path / "resnet18.pth")
    torch.save(m.state_dict(), path)
    img = ops.synth_images(0, 0, 4, DEV)
    ex = HipExecutor(DEV, seed=5, weights={"resnet": path})
    try:
        r = ex.runner("resnet18")
        assert r.split and r._split_ok()
        assert torch.equal(r.logits(img), _runner(P.compile_model(m, "resnet18", "fp32"), "fp32").logits(img))
        cls, prob = ex.run("resnet18", img, 0, 3, topk=5)                # captures and replays the top-k graph
        assert r.has_graph(4, slot=0, topk=5) or r.has_graph(4, slot=1, topk=5)
        assert not r.has_graph(4, slot=0) and not r.has_graph(4, slot=1)  # a graph of its own
        assert cls.shape == (4, 5) and cls.dtype == np.int32 and prob.shape == (4, 5) and prob.dtype == np.float32
        ce, pe = r.forward(img, topk=5)                                  # eager
        assert np.array_equal(cls, ce.cpu().numpy())
        assert np.array_equal(prob.view(np.int32), pe.cpu().numpy().view(np.int32))
        c2, p2 = ex.run("resnet18", img, 0, 3, topk=5)                   # the other slot's graph, or a replay
        assert np.array_equal(c2, cls) and np.array_equal(p2.view(np.int32), prob.view(np.int32))
        c1, p1 = ex.run("resnet18", img, 0, 3)                           # today's path
        assert c1.shape == (4,) and np.array_equal(cls[:, 0], c1)
        assert np.array_equal(prob[:, 0].view(np.int32), p1.view(np.int32))
        idx, v = _stable_ref(r.logits(img), 5)
        assert np.array_equal(cls, idx.numpy())
        assert torch.allclose(torch.from_numpy(prob).double(), v, rtol=1e-5, atol=1e-7)
        # what topk cannot be combined with
        packed = torch.zeros(4, 2, dtype=torch.int32, device=DEV)
        with pytest.raises(ValueError, match="packed"):
            r.forward(img, packed=packed, topk=5)
        with pytest.raises(ValueError, match="packed"):
            r.capture(4, packed=packed, topk=5)
        with pytest.raises(ValueError, match="capture_window"):
            r.capture_window(img, 2, topk=5)
        for bad in (0, 17, 2.5):
            with pytest.raises(ValueError, match="topk"):
                ex.run("resnet18", img, 0, 3, topk=bad)
    finally:
        ex.close()


def test_guard_rerun_serves_topk_from_a_checkpoint(ops, tmp_path):
    """The module of tests/test_split.py::test_split_activations_past_fp16_range_match_fp64
    as a checkpoint: the top-k graph marks the chunk, the executor reruns it on
    the f32 kernels and still returns [n, k] results."""
    from idunno.runtime.executor import HipExecutor

    m = ref.build("resnet18", seed=3)
    with torch.no_grad():
        m.conv1.weight *= 1e5
    path = str(tmp_path / "big.pth")
    torch.save(m.state_dict(), path)
    img = ops.synth_images(4, 0, 4, DEV)
    with torch.no_grad():
        want = m.double()(ref.preprocess_u8(img.cpu()).double())
    ex = HipExecutor(DEV, weights={"resnet18": path})
    try:
        r = ex.runner("resnet18")
        assert r.split and r._split_ok()
        sin, replay = r.capture(4, topk=5)                               # the graph itself marks every entry
        sin.copy_(img)
        cg, pg = replay()
        assert cg.shape == (4, 5) and bool((cg == ops.OVERFLOW_CLASS).all()) and bool((pg == 0).all())
        before = r.overflow_reruns
        cls, prob = ex.run("resnet18", img, 0, 3, topk=5)
        assert r.overflow_reruns == before + 1
        assert cls.shape == (4, 5) and prob.shape == (4, 5)
        assert not (cls == ops.OVERFLOW_CLASS).any() and (cls >= 0).all() and (cls < 1000).all()
        assert np.array_equal(cls[:, 0], want.argmax(1).numpy())
        assert (prob[:, :-1] >= prob[:, 1:]).all() and np.isfinite(prob).all()
        assert all(len(set(row.tolist())) == 5 for row in cls)
        assert abs(float(prob[0, 0]) - torch.softmax(want, 1).max(1).values[0].item()) < 1e-4
        ce, _ = r.forward(img, topk=5)                                   # the eager forward reruns by itself
        assert np.array_equal(ce.cpu().numpy(), cls)
    finally:
        ex.close()
