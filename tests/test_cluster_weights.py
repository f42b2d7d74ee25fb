"""Checkpoints in the cluster: nodes whose executors serve a checkpoint answer
a query with the classes the checkpointed module itself gives, and
``ClusterConfig.weights`` loads from file, environment and override."""
import json

import pytest
import torch

from idunno.config import ClusterConfig
from idunno.launch import build_parser, parse_weights
from idunno.models import reference as ref
from idunno.runtime.cluster import LocalCluster
from idunno.runtime.data import SyntheticSource, synth_images_cpu
from idunno.runtime.executor import TorchExecutor

FAST = dict(heartbeat_period_s=0.05, failure_timeout_s=1.0, metadata_period_s=0.1, rpc_timeout_s=2.0)
DATA_SEED = 1234


def _diverse_module(n):
    """BN-randomised ResNet18 whose logits are centred and stretched over the ``n``
    query images: a random-init net would send every image to one class, and a
    node serving the wrong parameters could then still answer "right"."""
    m = ref.build("resnet18", seed=3, randomize_bn=True)
    x = ref.preprocess_u8(torch.from_numpy(synth_images_cpu(DATA_SEED, 0, n)))
    with torch.no_grad():
        z = m(x)
        m.fc.weight *= 20.0
        m.fc.bias.copy_(20.0 * (m.fc.bias - z.mean(0)))
        cls = m(x).argmax(1)
    return m, cls.tolist()


def test_cluster_serves_the_checkpoint(tmp_path, monkeypatch):
    monkeypatch.delenv("IDUNNO_CLASSES", raising=False)
    m, want = _diverse_module(12)
    assert len(set(want)) >= 3                          # the query has more than one answer
    path = str(tmp_path / "resnet18.pth")
    torch.save(m.state_dict(), path)
    c = LocalCluster(num_nodes=3, executor_factory=lambda i: TorchExecutor(weights={"resnet18": path}),
                     source_factory=lambda i, node: SyntheticSource(DATA_SEED), **FAST).start()
    try:
        cl = c.client()
        cl.inference(0, 11, "resnet18")
        s = cl.wait_idle(60, {"resnet18": 12})
        assert s["done"]["resnet18"] == 12 and s["pending"] == 0
        got = {}
        for k, chunks in cl.view("c4")["results"].items():
            assert k.startswith("resnet18 ")
            for ch in chunks:
                for name, cat, p in eval(ch):           # reference string format: top-1 triples
                    got[int(name[5:-5])] = int(cat.split("_")[1])
                    assert 0.0 < p <= 1.0
        assert [got[i] for i in range(12)] == want
        # every node that worked loaded the file itself
        assert sum("resnet18" in n.executor.models for n in c.nodes.values()) >= 2
    finally:
        c.stop()
    # the seed's parameters answer differently: the classes above came from the file
    seed = TorchExecutor(seed=0).run("resnet18", SyntheticSource(DATA_SEED).get(0, 11), 0, 11)[0]
    assert seed.tolist() != want


def test_config_weights_file_env_override(tmp_path):
    assert ClusterConfig().weights == {} and ClusterConfig.load(env={}).weights == {}
    f = tmp_path / "cfg.json"
    f.write_text(json.dumps({"weights": {"resnet18": "/file/r18.pth"}, "num_nodes": 3}))
    assert ClusterConfig.load(str(f), env={}).weights == {"resnet18": "/file/r18.pth"}
    env = {"IDUNNO_WEIGHTS": '{"resnet18": "/env/r18.pth", "alexnet": "/env/a.pth"}'}
    cfg = ClusterConfig.load(str(f), env=env)
    assert cfg.weights == {"resnet18": "/env/r18.pth", "alexnet": "/env/a.pth"} and cfg.num_nodes == 3
    cfg = ClusterConfig.load(str(f), env=env, weights={"resnet50": "/cli/r50.pth"})
    assert cfg.weights == {"resnet50": "/cli/r50.pth"}
    assert cfg.to_dict()["weights"] == {"resnet50": "/cli/r50.pth"}
    a, b = ClusterConfig(), ClusterConfig()
    a.weights["x"] = "y"
    assert b.weights == {}                              # no shared default


def test_launch_weights_flag(tmp_path):
    a = build_parser().parse_args(["cluster", "--weights", "resnet=a.pth", "--weights", "alexnet=/w/b.safetensors"])
    assert a.weights == ["resnet=a.pth", "alexnet=/w/b.safetensors"]
    w = parse_weights(a.weights)
    assert set(w) == {"resnet18", "alexnet"} and w["alexnet"] == "/w/b.safetensors" and w["resnet18"].endswith("/a.pth")
    assert build_parser().parse_args(["node"]).weights is None and parse_weights(None) == {}
    for bad in ("resnet18", "=x.pth", "resnet18="):
        with pytest.raises(ValueError, match="MODEL=PATH"):
            parse_weights([bad])
    with pytest.raises(ValueError, match="unknown model"):
        parse_weights(["vgg=x.pth"])
