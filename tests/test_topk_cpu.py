"""Top-k results and checkpoints through TorchExecutor, deeplearning() and the
inference command line, on the CPU.  The order under test is the stable
descending sort (value descending, then class index ascending); torch.topk
does not promise that order, so the oracles here sort."""
import os

import numpy as np
import pytest
import torch

from idunno import inference
from idunno.models import reference as ref
from idunno.runtime.data import SyntheticSource, synth_images_cpu
from idunno.runtime.executor import FakeExecutor, TorchExecutor, make_executor, stable_topk

NEG = float("-inf")


def stable_order(row):
    """Indices of a python stable sort: value descending, then index ascending."""
    return sorted(range(len(row)), key=lambda i: (-row[i], i))


def test_stable_topk_tie_cases():
    # the case torch.topk orders differently on some builds: the three 5s in index order, then the 2s
    z = torch.tensor([[1.0, 5.0, 5.0, 2.0, 5.0, NEG, 2.0]])
    cls, prob = stable_topk(z, 5)
    assert cls.dtype == torch.int32 and cls.tolist() == [[1, 2, 4, 3, 6]]
    assert stable_order(z[0].tolist())[:5] == [1, 2, 4, 3, 6]
    p = torch.softmax(z.double(), 1)[0]
    assert torch.allclose(prob[0].double(), p[[1, 2, 4, 3, 6]], rtol=1e-6, atol=0)
    # the tie straddles k: the lower index is in, the higher one out
    assert stable_topk(z, 2)[0].tolist() == [[1, 2]]
    # fewer finite entries than k: the -inf entries follow in index order, probability 0
    z = torch.tensor([[NEG, 3.0, NEG, NEG, 1.0]])
    cls, prob = stable_topk(z, 4)
    assert cls.tolist() == [[1, 4, 0, 2]] and prob[0, 2:].tolist() == [0.0, 0.0]
    for bad in (0, 17, 6, 2.5, True):
        with pytest.raises(ValueError, match="topk"):
            stable_topk(torch.zeros(1, 5 if bad == 6 else 40), bad)


@pytest.fixture(scope="module")
def served(tmp_path_factory):
    """A BN-randomised ResNet18 saved as a checkpoint, 4 images, and the module's own fp32 outputs."""
    d = tmp_path_factory.mktemp("ckpt")
    m = ref.build("resnet18", seed=3, randomize_bn=True)
    path = str(d / "resnet18.pth")
    torch.save(m.state_dict(), path)
    img = torch.from_numpy(synth_images_cpu(1234, 0, 4))
    with torch.no_grad():
        z = m(ref.preprocess_u8(img))
    return path, img, z, torch.softmax(z, 1)


def test_torch_executor_serves_the_checkpoint_topk(served):
    path, img, z, p = served
    ex = TorchExecutor(weights={"resnet": path})          # an alias: keys are canonicalised
    cls, prob = ex.run("resnet18", img, 0, 3, topk=5)
    assert cls.shape == (4, 5) and cls.dtype == np.int32 and prob.shape == (4, 5) and prob.dtype == np.float32
    order = torch.sort(p, dim=1, descending=True, stable=True).indices[:, :5]
    assert np.array_equal(cls, order.numpy())
    assert [stable_order(z[i].tolist())[:5] for i in range(4)] == cls.tolist()
    assert np.array_equal(prob, p.gather(1, order).numpy())
    # column 0 is run() without topk, and submit() hands topk on
    c1, p1 = ex.run("resnet18", img, 0, 3)
    assert c1.shape == (4,) and np.array_equal(cls[:, 0], c1) and np.array_equal(prob[:, 0], p1)
    cs, ps = ex.submit("resnet18", img, 0, 3, topk=5).result()
    assert np.array_equal(cs, cls) and np.array_equal(ps, prob)
    assert np.array_equal(ex.submit("resnet18", img, 0, 3).result()[0], c1)
    # the checkpoint, not the seed: a model absent from ``weights`` keeps the seed's parameters
    with torch.no_grad():
        seed0 = torch.softmax(ref.build("resnet18", seed=0)(ref.preprocess_u8(img)), 1).max(1).values
    assert not np.allclose(p1, seed0.numpy())
    assert np.array_equal(TorchExecutor(seed=0).run("resnet18", img, 0, 3)[1], seed0.numpy())
    with pytest.raises(ValueError, match="topk"):
        ex.run("resnet18", img, 0, 3, topk=17)


def test_make_executor_and_fake_executor(served):
    path, img, _, p = served
    ex = make_executor("torch", weights={"resnet18": path})
    assert np.array_equal(ex.run("resnet18", img, 0, 3)[1], p.max(1).values.numpy())
    with pytest.raises(ValueError, match="unknown model"):
        make_executor("torch", weights={"vgg": path})
    f = make_executor("fake", weights={"resnet18": path})                    # stays as it is
    assert isinstance(f, FakeExecutor) and f.run("resnet18", None, 0, 3)[0].shape == (4,)


def test_deeplearning_topk_weights_classes(served, tmp_path, monkeypatch):
    path, img, z, p = served
    monkeypatch.delenv("IDUNNO_CLASSES", raising=False)
    classes = tmp_path / "names.txt"
    classes.write_text("".join(f"cat {i}\n" for i in range(1000)))
    assert np.array_equal(SyntheticSource(1234).get(0, 3).numpy(), img.numpy())
    # topk=1 (the default): today's 3-tuples
    res, dt = inference.deeplearning("no_such_dir", "resnet18", 0, 3, device="cpu", weights=path, topk=1)
    assert dt > 0 and len(res) == 4
    top = p.max(1)
    for i, r in enumerate(res):
        assert r == (f"test_{i}.JPEG", f"class_{int(top.indices[i])}", float(top.values[i]))
    assert res == inference.deeplearning("no_such_dir", "resnet18", 0, 3, device="cpu", weights=path)[0]
    # topk=5: tuples of names and probabilities, names from the classes file
    res5, _ = inference.deeplearning("no_such_dir", "resnet", 0, 3, device="cpu", weights=path, topk=5,
                                     classes=str(classes))
    assert len(res5) == 4
    for i, (name, cats, probs) in enumerate(res5):
        want = stable_order(z[i].tolist())[:5]
        assert name == f"test_{i}.JPEG" and cats == tuple(f"cat {c}" for c in want)
        assert isinstance(probs, tuple) and probs == tuple(float(p[i, c]) for c in want)
        assert probs[0] == res[i][2] and all(a >= b for a, b in zip(probs, probs[1:]))
    # without weights: the seed's parameters, as before
    r0, _ = inference.deeplearning("no_such_dir", "resnet18", 0, 1, device="cpu")
    assert len(r0[0]) == 3 and isinstance(r0[0][1], str) and r0[0][2] != res[0][2]
    for bad in (0, 17, 2.0, True):
        with pytest.raises(ValueError, match="topk"):
            inference.deeplearning("no_such_dir", "resnet18", 0, 1, device="cpu", topk=bad)


def test_deeplearning_reloads_a_replaced_checkpoint(served, tmp_path):
    src, img, _, p = served
    path = str(tmp_path / "w.pth")
    m = ref.build("resnet18", seed=8, randomize_bn=True)
    torch.save(m.state_dict(), path)
    with torch.no_grad():
        p8 = torch.softmax(m(ref.preprocess_u8(img)), 1).max(1).values
    r, _ = inference.deeplearning("no_such_dir", "resnet18", 0, 3, device="cpu", weights=path)
    assert [x[2] for x in r] == p8.tolist()
    n = len(inference._EXECUTORS)
    inference.deeplearning("no_such_dir", "resnet18", 0, 3, device="cpu", weights=path)
    assert len(inference._EXECUTORS) == n                         # the same file: the cached executor
    with open(src, "rb") as f:
        data = f.read()
    with open(path, "wb") as f:
        f.write(data)
    st = os.stat(path)
    os.utime(path, ns=(st.st_atime_ns, st.st_mtime_ns + 1_000_000_000))
    r, _ = inference.deeplearning("no_such_dir", "resnet18", 0, 3, device="cpu", weights=path)
    assert [x[2] for x in r] == p.max(1).values.tolist()


def test_inference_cli_arguments_round_trip(served, tmp_path, capsys):
    ap = inference.build_parser()
    a = ap.parse_args(["resnet18", "0", "3"])
    assert (a.topk, a.weights, a.classes) == (1, None, None)
    a = ap.parse_args(["resnet18", "0", "3", "--topk", "5", "--weights", "w.pth", "--classes", "c.txt"])
    assert (a.model, a.start, a.end, a.topk, a.weights, a.classes) == ("resnet18", 0, 3, 5, "w.pth", "c.txt")
    path = served[0]
    assert inference.main(["resnet18", "0", "1", "--device", "cpu", "--topk", "2", "--weights", path,
                           "--dir", str(tmp_path / "none")]) == 0
    import json

    rows = [json.loads(ln) for ln in capsys.readouterr().out.splitlines()]
    assert len(rows) == 2 and rows[0][0] == "test_0.JPEG" and len(rows[0][1]) == 2 and len(rows[0][2]) == 2
