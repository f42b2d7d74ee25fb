"""The decoder's four opt-ins (progressive, restart intervals, sampling, colorspace) in every
combination on one mixed batch, on the host: no option may act as another anywhere between
runtime/jpeg.py and the parser and packer.  For each combination the batch says which files
must be taken, why the others are refused, and which kernel the packer routes each one to."""
import pytest
from jpeg_options_cases import (EMPTY, NONE, NOT_JPEG, PARSER_OPTIONS, PNG, C, P, S, datas, jpegs, strings, subsets,
                                verdict)

from idunno import ops
from idunno.runtime import jpeg

ALL_OPTIONS = ("progressive", "restart", "sampling", "colorspace")


@pytest.mark.parametrize("enabled", subsets(PARSER_OPTIONS), ids=lambda e: "+".join(sorted(e)) or "none")
def test_the_parser_takes_exactly_what_its_options_admit(enabled):
    flags = (P in enabled, S in enabled, C in enabled)
    kw = strings(enabled)
    del kw["restart"]
    status = list(ops.jpeg_entropy_batch(datas(), 2, *flags)[0])
    assert status[PNG] == NOT_JPEG and status[NONE] == EMPTY
    for i, name, d, needs, _ in jpegs():
        ok, reason = verdict(needs, enabled)
        st, why, hdr = ops.jpeg_parse(d, *flags)
        assert (st == 0, why) == (ok, reason) and (hdr is not None) == ok, (name, st, why)
        got = jpeg.parse(d, **kw)
        assert (isinstance(got, dict), got if isinstance(got, str) else "ok") == (ok, reason), (name, got)
        assert (status[i] == 0) == ok and status[i] == st, (name, status[i])


@pytest.mark.parametrize("parallel", (False, True))
@pytest.mark.parametrize("enabled", subsets(ALL_OPTIONS), ids=lambda e: "+".join(sorted(e)) or "none")
def test_the_packer_remembers_its_options_and_routes_by_them(enabled, parallel):
    flags = (P in enabled, "restart" in enabled, S in enabled, C in enabled)
    pk = ops.jpeg_huff_pack(datas(), parallel, *flags)
    assert (pk.native_progressive, pk.restart_intervals, pk.native_sampling, pk.native_colorspace) == flags
    assert pk.parallel is parallel and pk.status[PNG] == NOT_JPEG and pk.status[NONE] == EMPTY
    count = {"lane": 0, "par": 0, "prog": 0, "rst": 0}
    for i, name, _, needs, kind in jpegs():
        ok, _ = verdict(needs, enabled)
        assert (pk.status[i] == 0) == ok and (pk.offs[i] >= 0) == ok, (name, pk.status[i])
        if not ok:
            continue
        if kind == "progressive":
            count["prog"] += 1
        elif kind == "four":
            count["lane"] += 1
        elif kind == "restart":
            count["rst" if "restart" in enabled else "lane"] += 1
        else:
            count["par" if parallel else "lane"] += 1
    assert (pk.n_lane, pk.n_par, pk.n_prog, pk.n_rst) == (count["lane"], count["par"], count["prog"], count["rst"])
    assert pk.n_gpu == sum(count.values())


@pytest.mark.parametrize("form", jpeg.ENTROPY_ON, ids=lambda f: "prepared_" + f)    # no id that is a marker's name
def test_a_prepared_entropy_stage_echoes_its_options_and_decides_them(form):
    other_form = "gpu" if form == "host" else "host"
    for enabled in subsets(ALL_OPTIONS):
        kw = strings(enabled)
        ent = jpeg.entropy_batch(datas(), 2, form, **kw)
        assert ent.form == form and ent.datas == datas()
        assert (ent.options.progressive, ent.options.restart, ent.options.sampling, ent.options.colorspace) == (
            kw["progressive"], kw["restart"], kw["sampling"], kw["colorspace"])
        for i, name, _, needs, _ in jpegs():
            assert (ent.status[i] == 0) == verdict(needs, enabled)[0], (name, ent.status[i])
        # decode_batch asked for the opposite of everything: what was prepared decides, but for restart in
        # the host form, which does nothing with it and reports the one asked for
        opposite = strings(frozenset(ALL_OPTIONS) - enabled)
        _, info = jpeg.decode_batch(datas(), "cpu", resize=None, crop=None, entropy=ent, entropy_on=other_form, **opposite)
        want = dict(kw, entropy_on=form)
        if form == "host":
            want["restart"] = opposite["restart"]
        assert {k: info[k] for k in want} == want, (enabled, info)
        assert [info[k + "_images"] for k in ALL_OPTIONS] == [0, 0, 0, 0]


def test_every_option_combination_is_covered():
    assert len(subsets(PARSER_OPTIONS)) == 8 and len(set(subsets(ALL_OPTIONS))) == 16
    assert {tuple(sorted(n)) for _, _, _, n, _ in jpegs()} == {(), (P,), (S,), (C,), (P, S), (C, P)}
