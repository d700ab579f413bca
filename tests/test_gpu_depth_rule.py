"""The emission kernels (vgmi_hmm.hip: hmm_emissions_kernel, hmm_emissions_win_kernel, every instantiation vgmi_api_hmm.cpp launches) over
the whole domain of the depth rule: every coverage 0 .. 255, every multiplicity 1 .. 255, the flag bit, a carrier on the genotypes and one
on none, every copy number the ploidy allows inside and outside the interval -- 261 120 rows of one entry each, at every average and
interval of tests/golden/depth_rule.npz.  The term table is tables[i] = i + 1, so a row's score is the index of the term the kernel picked,
plus one; the indices, n_kept and the flag bytes are compared with tests/depth_rule_cases.py's expected(), which reads the table the
reference's own find_most_likely_depth recorded (tests/test_depth_rule_cpu.py holds the numpy model to the same table and shows which
mistakes these cases tell apart).

A family's entries do not depend on the case: they are uploaded once, to one context the module keeps, and a test is one call."""
import functools

import numpy as np
import pytest

from varigraph_amd import vgmi
import depth_rule_cases as D

pytestmark = pytest.mark.gpu

LD = np.longdouble


@functools.lru_cache(maxsize=None)
def _rows():
    return D.rows()


@functools.lru_cache(maxsize=2)
def _inputs(fam):
    return D.family_inputs(fam, _rows())


@pytest.fixture(scope="module")
def device():
    """one context for the module; `uploaded`: the family whose entries it holds"""
    state = dict(ctx=vgmi.Context(0, buffer_mib=16), uploaded=None)
    try:
        yield state
    finally:
        state["ctx"].close()


def _run(state, fam, ave, lower, upper):
    ctx, x, tables = state["ctx"], _inputs(fam), D.term_tables(fam.ploidy)
    rows = (x["entry_begin"], x["entry_count"])
    if fam.kind in ("emissions", "emissions_pos"):      # (the call uploads its entries itself)
        state["uploaded"] = None
        top = sum(int(w) << (64 * i) for i, w in enumerate(x["top_words"][0]))
        a = (x["words"], x["cov"], x["used"], x["pos"][:, 0], x["pos"][:, 1], top, fam.bit_len, ave, lower, upper, tables, *rows, x["gt0_places"])
        return ctx.hmm_emissions(*a, pos=x["pos"] if fam.kind == "emissions_pos" else None), None
    wide = fam.kind.endswith("_wide")
    if state["uploaded"] != fam.name:
        state["uploaded"] = None
        if wide:
            ctx.hmm_entries_upload_wide(x["f"], x["bits"], fam.bit_len, x["cov"])
        else:
            ctx.hmm_entries_upload(x["words"], x["cov"])
        state["uploaded"] = fam.name
    top = x["top_words"] if wide else x["top_words"][:, 0]
    if fam.kind in ("select", "select_wide"):
        call = ctx.hmm_emissions_select_wide if wide else ctx.hmm_emissions_select
        got = call(x["pos"][:, 0], x["pos"][:, 1], [x["used"]], top, fam.bit_len, ave, lower, upper, tables, *rows, x["row_win"], x["gt0_places"])
    else:
        call = ctx.hmm_emissions_select_ploidy_wide if wide else ctx.hmm_emissions_select_ploidy
        gt0 = x["gt0_words"] if wide else x["gt0_words"][:, 0]
        got = call(fam.ploidy, x["win_n_gt"], x["win_haps"], top, fam.bit_len, ave, lower, upper, tables, *rows, x["row_win"], gt0)
    return got, ctx.hmm_alive_fetch()


@pytest.mark.parametrize("case", D.CASE_NAMES)
@pytest.mark.parametrize("fam", D.FAMILIES, ids=[f.name for f in D.FAMILIES])
def test_every_row_picks_the_reference_s_term(device, fam, case):
    assert np.finfo(LD).nmant == 63, "numpy.longdouble is not the x87 format here"
    ave, lower, upper, table = D.golden()[case]
    r = _rows()
    want_idx, want_kept, want_flags = D.expected(r, fam.ploidy, table, lower, upper)
    (obs, n_kept, flags), alive = _run(device, fam, float(ave), lower, upper)
    assert obs.shape == want_idx.shape and obs.dtype == LD
    picked = obs - LD(1)      # 1.0L * tables[i] is stored as tables[i] = i + 1, exactly
    idx = picked.astype(np.int64)
    assert np.array_equal(idx.astype(LD), picked), "a score that is no whole number"
    bad = np.argwhere(idx != want_idx)
    assert bad.size == 0, (len(bad), [dict(c=int(r.c[i]), f=int(r.f[i]), flag=int(r.flag[i]), carrier=int(r.carrier[i]), genotype=int(g), got=int(idx[i, g]),
                                           want=int(want_idx[i, g])) for i, g in bad[:8]])
    assert n_kept.dtype == np.uint32 and np.array_equal(n_kept, want_kept)
    bad = np.flatnonzero(flags != want_flags)
    assert flags.dtype == np.uint8 and bad.size == 0, (len(bad), [(int(r.c[i]), int(r.f[i]), int(r.flag[i]), int(r.carrier[i]), int(flags[i])) for i in bad[:8]])
    if alive is not None:      # an entry some drawn haplotype carries stays in its list
        assert alive.size == r.c.size and alive.all()
