"""``restart="intervals"`` without a GPU: what the packer lays out for the interval
kernel (which files it takes, one work item per restart interval, the mutants it
leaves to the one-lane kernel), that nothing changes without the option, and the
option's validation, CPU-device behaviour and command-line flags."""
import collections

import pytest
import torch
from jpeg_cases import encode, png
from jpeg_prog_cases import named
from jpeg_restart_cases import SPEC, files, mutant_fill, refused_mutants, table

from idunno.runtime import jpeg


def _ops():
    from idunno import ops

    ops.load()
    return ops


def _batch():
    """The table's files, then a file without a restart interval, a progressive file with restart
    markers, None and a PNG."""
    return files() + [encode(38, 30, "420", 75, seed=2), named("70x46-420-rst3")[1], None, png()]


@pytest.mark.parametrize("par", [False, True])
def test_packer_takes_every_table_file_one_item_per_interval(par):
    ops = _ops()
    datas = _batch()
    nt = len(table())
    pk = ops.jpeg_huff_pack(datas, par, False, True)
    assert pk.restart_intervals is True and pk.parallel is par
    assert pk.n_rst == nt and pk.n_prog == 0
    assert (pk.n_par, pk.n_lane) == ((1, 0) if par else (0, 1))        # the file without a restart interval
    assert pk.n_gpu == nt + 1
    assert list(pk.status[:nt + 1]) == [0] * (nt + 1) and all(s != 0 for s in pk.status[nt + 1:])
    items = pk.rst_items
    assert items.dtype == torch.int32 and items.dim() == 2 and items.shape[1] == 4
    per = collections.Counter(items[:, 0].tolist())
    assert [per[i] for i in range(nt)] == [k for _, k in table()] and set(per) == set(range(nt))
    at = 0
    for i, ((d, k), (w, h, sub, kw, _)) in enumerate(zip(table(), SPEC)):
        rows = items[at:at + k].tolist()
        at += k
        hdr = jpeg.parse(d)
        ri = hdr["restart_interval"]
        assert ri > 0
        scan = d.index(b"\xff\xda")
        scan += 2 + (d[scan + 2] << 8 | d[scan + 3])
        for j, (entry, begin, mcu, index) in enumerate(rows):
            assert (entry, mcu, index) == (i, j * ri, j)
            # an interval starts right after RST((j - 1) mod 8), the first one at the scan's first byte
            assert begin == 0 if j == 0 else d[scan + begin - 2:scan + begin] == bytes([0xFF, 0xD0 + (j - 1) % 8])
    assert at == items.shape[0]
    # the progressive file is the progressive kernel's, with or without the option
    pk = ops.jpeg_huff_pack(datas, par, True, True)
    assert pk.n_rst == nt and pk.n_prog == 1 and (pk.n_par, pk.n_lane) == ((1, 0) if par else (0, 1))


@pytest.mark.parametrize("par", [False, True])
def test_without_the_option_the_packed_batch_is_todays(par):
    ops = _ops()
    datas = _batch()
    nt = len(table())
    for pk in (ops.jpeg_huff_pack(datas, par, False), ops.jpeg_huff_pack(datas, par, False, False)):
        assert pk.restart_intervals is False and pk.n_rst == 0 and pk.rst_items.shape[0] == 0
        assert (pk.n_par, pk.n_lane) == ((1, nt) if par else (0, nt + 1)) and pk.n_gpu == nt + 1
    a, b = ops.jpeg_huff_pack(datas, par, False, False), ops.jpeg_huff_pack(datas, par, False, True)
    assert torch.equal(a.bytes, b.bytes) and a.offs == b.offs and a.status == b.status      # the same layout


def test_refused_mutants_stay_on_the_one_lane_kernel():
    ops = _ops()
    with_marker = [d for d, k in table() if k > 1]
    assert len(with_marker) == 8
    for d in with_marker:
        bad = [m for _, m in refused_mutants(d)]
        host = jpeg.entropy_coefs([d, mutant_fill(d)] + bad)[0]
        assert host == [0, 0, 3, 3, 3, 3]                              # the host decoder's verdicts
        assert [name for name, _ in refused_mutants(d)] == ["rst1", "removed", "data-byte", "cut"]
        for par in (False, True):
            pk = ops.jpeg_huff_pack([d, mutant_fill(d)] + bad, par, False, True)
            # a marker that is out of sequence, missing or cut is one the byte scan does not find: the file
            # stays with the one-lane kernel.  A data byte in front of an intact marker is invisible to a
            # byte scan (every marker is there, in sequence): that file is laid out for the interval kernel,
            # whose lane refuses it at the marker as the serial decoder does.
            assert pk.n_rst == 3 and pk.n_lane == 3 and pk.n_par == 0
            assert sorted(set(pk.rst_items[:, 0].tolist())) == [0, 1, 4]


def test_unknown_restart_is_refused_everywhere():
    from idunno import inference
    from idunno.runtime.data import GpuJpegSource

    assert jpeg.RESTART == ("lane", "intervals")
    p = files()[0]
    for bad in ("Intervals", "", "interval", "gpu"):
        for call in (lambda: jpeg.entropy_batch([p], 1, restart=bad),
                     lambda: jpeg.entropy_coefs([p], restart=bad),
                     lambda: jpeg.decode_batch([p], "cpu", restart=bad),
                     lambda: jpeg.decode_batch([p], "cuda", entropy_on="gpu", restart=bad),    # before a device is touched
                     lambda: GpuJpegSource("cpu", root=".", restart=bad),
                     lambda: inference.deeplearning("alexnet", "alexnet", 0, 0, device="cpu", restart=bad)):
            with pytest.raises(ValueError):
                call()


def test_mode_is_reported_and_ignored_on_a_cpu_device(tmp_path):
    from idunno.runtime.data import GpuJpegSource

    datas = files()[:3] + [None]
    base, binfo = jpeg.decode_batch(datas, "cpu")
    assert binfo["restart"] == "lane" and binfo["restart_images"] == 0
    for form in jpeg.ENTROPY_ON:
        imgs, info = jpeg.decode_batch(datas, "cpu", entropy_on=form, restart="intervals")
        assert info["restart"] == "intervals" and info["restart_images"] == 0
        assert [r for _, r in info["fallbacks"]] == ["cpu_device"] * 3 and torch.equal(imgs, base)
    # the host form: the same coefficients, whatever the option
    a = jpeg.entropy_coefs(files(), restart="intervals")
    b = jpeg.entropy_coefs(files())
    assert a[0] == b[0] == [0] * len(files()) and a[1] == b[1] and torch.equal(a[2], b[2])
    for i in range(3):
        (tmp_path / f"test_{i}.JPEG").write_bytes(datas[i])
    src = GpuJpegSource("cpu", root=str(tmp_path), entropy_on="gpu_parallel", restart="intervals")
    assert src.restart == "intervals" and torch.equal(src.get(0, 2), base[:3]) and src.restart_images == 0
    assert GpuJpegSource("cpu", root=str(tmp_path)).restart == "lane"


def test_command_lines_pass_the_mode_on(monkeypatch):
    from idunno import inference, launch

    seen = []

    def fake(filename, modelname, start, end, **kw):
        seen.append(kw["restart"])
        return [], 0.0

    monkeypatch.setattr(inference, "deeplearning", fake)
    assert inference.main(["alexnet", "0", "0", "--decoder", "gpu", "--entropy", "gpu", "--restart", "intervals"]) == 0
    assert inference.main(["alexnet", "0", "0"]) == 0
    assert seen == ["intervals", "lane"]
    with pytest.raises(SystemExit):
        inference.main(["alexnet", "0", "0", "--restart", "rows"])
    ap = launch.build_parser()
    assert ap.parse_args(["node"]).jpeg_restart == "lane"
    assert ap.parse_args(["cluster", "--source", "jpeg", "--jpeg-restart", "intervals"]).jpeg_restart == "intervals"
    with pytest.raises(SystemExit):
        ap.parse_args(["node", "--jpeg-restart", "rows"])
    # a cluster forwards the flag to its child nodes, and a node hands it to its source
    started = []

    class FakeProc:
        def __init__(self, cmd, **kw):
            started.append(cmd)

        def wait(self, timeout=None):
            return 0

        def poll(self):
            return 0

    monkeypatch.setattr(launch.subprocess, "Popen", FakeProc)
    assert launch.main(["cluster", "--nodes", "2", "--no-shell", "--source", "jpeg", "--jpeg-entropy", "gpu",
                        "--jpeg-restart", "intervals"]) == 0
    assert len(started) == 2
    for cmd in started:
        assert cmd[cmd.index("--jpeg-restart") + 1] == "intervals"
    import inspect

    assert "restart=a.jpeg_restart" in inspect.getsource(launch.run_node)
