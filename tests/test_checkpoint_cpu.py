"""models.checkpoint on the CPU: every supported file form of a state dict
loads into a fresh module that computes what the source module computes, bit
for bit; every malformed checkpoint is refused with a ValueError; a pickled
object is refused without being run."""
import os

import pytest
import torch

from idunno.models import build_program, compile_model
from idunno.models import checkpoint as ck
from idunno.models import reference as ref
from idunno.runtime.data import synth_images_cpu

NAMES = ("resnet18", "resnet50", "alexnet")


@pytest.fixture(scope="module")
def sources():
    """name -> (source module, its state dict, input, output); built once, never changed."""
    x = ref.preprocess_u8(torch.from_numpy(synth_images_cpu(5, 0, 2)))
    out = {}
    for name in NAMES:
        m = ref.build(name, seed=3, randomize_bn=True)
        with torch.no_grad():
            out[name] = (m, {k: v.clone() for k, v in m.state_dict().items()}, x, m(x))
    return out


def _forward(m, x):
    with torch.no_grad():
        return m(x)


def _save_forms(state, d):
    """(label, path) of each full-precision file form, written on demand and removed by the caller."""
    from safetensors.torch import save_file

    def pth(obj, fn):
        p = os.path.join(d, fn)
        torch.save(obj, p)
        return p

    yield "bare", pth(state, "bare.pth")
    yield "state_dict", pth({"state_dict": state, "epoch": 90}, "wrapped.pth")
    yield "model", pth({"model": state, "optimizer": {"lr": 0.1}}, "wrapped_model.pt")
    yield "module.", pth({"module." + k: v for k, v in state.items()}, "ddp.pth")
    p = os.path.join(d, "m.safetensors")
    save_file({k: v.contiguous() for k, v in state.items()}, p)
    yield "safetensors", p


@pytest.mark.parametrize("name", NAMES)
def test_every_file_form_round_trips_bit_equal(sources, tmp_path, name):
    m, state, x, want = sources[name]
    assert any(k.endswith("num_batches_tracked") for k in state) == name.startswith("resnet")
    for label, path in _save_forms(state, str(tmp_path)):
        got = ck.model_from_state(name, ck.load_state(path))
        os.unlink(path)
        assert not got.training
        assert torch.equal(_forward(got, x), want), label
    # a state dict handed over directly, and the digest of equal states
    got = ck.model_from_state(name, state)
    assert torch.equal(_forward(got, x), want)
    assert ck.state_digest(got) == ck.state_digest(m) == ck.state_digest(state)
    assert ck.state_digest(got) != ck.state_digest(ref.build(name, seed=0))


@pytest.mark.parametrize("name", NAMES)
def test_fp16_stored_checkpoint_is_cast_to_fp32(sources, tmp_path, name):
    m, state, x, _ = sources[name]
    half = {k: (v.half() if v.is_floating_point() else v) for k, v in state.items()}
    path = str(tmp_path / "half.pth")
    torch.save(half, path)
    got = ck.model_from_state(name, ck.load_state(path))
    os.unlink(path)
    assert all(p.dtype == torch.float32 for p in got.parameters())
    # the oracle: the source architecture with every tensor rounded through fp16
    rounded = ref.BUILDERS[name]()
    rounded.load_state_dict({k: (v.half().float() if v.is_floating_point() else v) for k, v in state.items()})
    assert torch.equal(_forward(got, x), _forward(rounded.eval(), x))


@pytest.mark.parametrize("cast", [torch.bfloat16, torch.float64])
def test_bf16_and_fp64_are_cast_to_fp32(sources, cast):
    _, state, _, _ = sources["resnet18"]
    st = ck.normalise_state({k: (v.to(cast) if v.is_floating_point() else v) for k, v in state.items()})
    assert all(v.dtype == torch.float32 for v in st.values())
    assert not any(k.endswith("num_batches_tracked") for k in st)
    assert torch.equal(st["conv1.weight"], state["conv1.weight"].to(cast).float())


def _r18(sources):
    return {k: v for k, v in sources["resnet18"][1].items()}


def test_refusals_name_the_model_and_the_keys(sources):
    st = _r18(sources)
    missing = dict(st)
    del missing["layer1.0.bn1.running_var"]
    with pytest.raises(ValueError, match=r"resnet18.*missing keys: layer1\.0\.bn1\.running_var"):
        ck.model_from_state("resnet18", missing)
    extra = dict(st, **{"layer9.0.weight": torch.zeros(1)})
    with pytest.raises(ValueError, match=r"resnet18.*unexpected keys: layer9\.0\.weight"):
        ck.model_from_state("resnet18", extra)
    shape = dict(st, **{"conv1.weight": torch.zeros(64, 3, 3, 3)})
    with pytest.raises(ValueError, match=r"resnet18.*shape mismatch: conv1\.weight"):
        ck.model_from_state("resnet18", shape)
    for bad in (float("nan"), float("inf")):
        w = st["layer2.0.conv1.weight"].clone()
        w[1, 2, 0, 0] = bad
        with pytest.raises(ValueError, match=r"resnet18.*non-finite values in: layer2\.0\.conv1\.weight"):
            ck.model_from_state("resnet18", dict(st, **{"layer2.0.conv1.weight": w}))
    head = dict(st, **{"fc.weight": torch.zeros(10, 512), "fc.bias": torch.zeros(10)})
    with pytest.raises(ValueError, match=r"resnet18.*10 classes.*1000"):
        ck.model_from_state("resnet18", head)
    # another architecture's checkpoint
    with pytest.raises(ValueError, match="resnet50.*missing keys"):
        ck.model_from_state("resnet50", st)
    with pytest.raises(ValueError, match="alexnet.*missing keys: features.0.weight"):
        ck.model_from_state("alexnet", st)
    a = dict(sources["alexnet"][1])
    a["classifier.6.weight"], a["classifier.6.bias"] = torch.zeros(21, 4096), torch.zeros(21)
    with pytest.raises(ValueError, match=r"alexnet.*21 classes"):
        ck.model_from_state("alexnet", a)
    with pytest.raises(ValueError, match="unknown model"):
        ck.model_from_state("vgg16", st)
    for junk in ({}, {"state_dict": 3}, {"epoch": 1}, [1, 2]):
        with pytest.raises(ValueError, match="state dict"):
            ck.normalise_state(junk)
    # a mixed prefix is not a uniform one: the keys stay as they are and are refused
    mixed = {("module." + k if i % 2 else k): v for i, (k, v) in enumerate(st.items())}
    with pytest.raises(ValueError, match="unexpected keys: module"):
        ck.model_from_state("resnet18", mixed)


class _Touch:
    """Unpickling this would create ``path``."""

    def __init__(self, path):
        self.path = path

    def __reduce__(self):
        return (open, (self.path, "w"))


def test_pickled_object_is_refused_and_not_run(sources, tmp_path):
    side = str(tmp_path / "side_effect")
    path = str(tmp_path / "evil.pth")
    torch.save({"state_dict": _r18(sources), "hook": _Touch(side)}, path)
    with pytest.raises(ValueError, match="weights-only"):
        ck.load_state(path)
    assert not os.path.exists(side)
    with pytest.raises(ValueError, match="weights-only"):
        build_program("resnet18", dtype="fp32", weights=path)
    assert not os.path.exists(side)
    # the same file read the unsafe way does run it: the refusal above is what kept it from running
    torch.load(path, map_location="cpu", weights_only=False)
    assert os.path.exists(side)


def _same_program(a, b):
    assert (a.name, a.kind, a.num_classes, a.dtype) == (b.name, b.kind, b.num_classes, b.dtype)
    ca, cb = list(a.all_convs()), list(b.all_convs())
    assert len(ca) == len(cb) > 0
    n = 0
    for x, y in zip(ca, cb):
        for f in ("cin", "cout", "kh", "kw", "stride", "pad", "relu", "small", "s_scale", "fs_scale"):
            assert getattr(x, f) == getattr(y, f), f
        for f in ("w", "b", "wino", "p3", "sw", "sp3", "fs", "fs_bias", "fs_psum"):
            tx, ty = getattr(x, f), getattr(y, f)
            assert (tx is None) == (ty is None), f
            if tx is not None:
                assert tx.dtype == ty.dtype and torch.equal(tx, ty), f
                n += 1
    return n


@pytest.mark.parametrize("name,dtype", [("resnet18", "fp32"), ("resnet18", "fp16"), ("alexnet", "fp32")])
def test_compiled_program_equals_the_source_modules(sources, tmp_path, name, dtype):
    m, state, _, _ = sources[name]
    path = str(tmp_path / "w.pth")
    torch.save(state, path)
    want = compile_model(m, name, dtype)
    assert _same_program(compile_model(ck.load_model(name, path), name, dtype), want) > 4
    _same_program(build_program(name, seed=99, dtype=dtype, weights=path), want)       # the seed is ignored
    _same_program(build_program(name, dtype=dtype, weights=state), want)               # a dict works as well
    other = build_program(name, seed=0, dtype=dtype)                                   # not the seed's program
    assert not torch.equal(next(other.all_convs()).w, next(want.all_convs()).w)
