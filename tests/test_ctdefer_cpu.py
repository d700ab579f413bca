"""The geometry of the deferred counter updates (ctd_scratch_bytes / ctd_layout, varigraph_amd/csrc/vgmi_ctdefer.hip) on the host:
regions that cover the table, fields that fit their bit widths, a scratch that holds its arrays, the reciprocal ctd_region_of
divides by -- at every region's edges, with Python integers.  No HIP call is made: runs without a GPU."""
import shutil

import pytest

from ctdefer_harness import build_harness, run_harness

N_CU = [256, 304, 64, 2]
N_COUNTS = [1, 300, 5_000, 65_537, 1_800_000, 8_388_608, 8_388_609, 25_600_000, 58_720_257, 67_108_864]
N_BYTES = [0, 45_000_000, 600_000_000, 3_624_000_000, 1 << 36]      # (2^36: cap reaches its 0xC0000000 clamp)
CTD_MAX_BINS, CTD_REGION_MAX, CTD_CHUNK, CAP_MAX = 2048, 32768, 256, 0xC0000000


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    return build_harness(tmp_path_factory.mktemp("ctdefer"))


def _geometry(exe, triples, env=None):
    rc, out, err = run_harness(exe, ["geometry"] + [v for t in triples for v in t], env=env)
    assert rc == 0 and len(out) == len(triples), err
    for g, t in zip(out, triples):
        assert (g["n_cu"], g["n_counts"], g["n_bytes"]) == tuple(t)
    return out


def _check(g, knobs=False):
    n_counts, n_bins, region, room, cap, n_wg = g["n_counts"], g["n_bins"], g["region"], g["room"], g["cap"], g["n_wg"]
    assert g["bytes"] > 0 and g["d_n_counts"] == n_counts, g
    assert n_bins * region >= n_counts and (n_bins - 1) * region < n_counts, g
    assert 256 <= region <= CTD_REGION_MAX and 1 <= n_bins <= CTD_MAX_BINS, g
    assert cap > 0 and cap % CTD_CHUNK == 0 and cap <= CAP_MAX, g
    assert 1 <= room <= cap, g
    assert n_wg >= 2 and n_wg % 2 == 0 and n_wg <= g["n_cu"], g
    if not knobs:      # a block's worth of records: one per 16 bytes of text
        assert cap >= min(CAP_MAX, g["n_bytes"] // 16), g
        assert room * n_bins * n_wg >= cap, g      # the rooms of all workgroups hold a full record buffer
    # the scratch holds its arrays, in order, none upon another
    assert g["cursor_at"] == 0 and g["bin_cursor_at"] == 4, g
    assert g["bin_cursor_end"] - g["bin_cursor_at"] == 4 * n_bins * n_wg, g
    assert g["bin_cursor_end"] <= g["rec_at"] and g["rec_at"] % 8 == 0, g
    assert g["rec_end"] - g["rec_at"] == 8 * cap and g["rec_end"] <= g["binned_at"] and g["binned_at"] % 4 == 0, g
    assert g["binned_end"] - g["binned_at"] == 4 * n_bins * n_wg * room and g["binned_end"] <= g["bytes"], g
    # ctd_region_of: (lo * inv) >> 32 is lo // region or one more (the kernel takes one off when it is too large)
    inv = g["inv"]
    assert 0 < inv < 1 << 32
    for b in range(n_bins + 1):
        for lo in (b * region - 1, b * region, b * region + region - 1):
            if 0 <= lo < n_counts:
                assert (lo * inv) >> 32 in (lo // region, lo // region + 1), (g, lo)
    assert ((n_counts - 1) * inv) >> 32 in (n_bins - 1, n_bins), g


@pytest.mark.parametrize("n_cu", N_CU)
def test_geometry_covers_the_table_and_fits_its_fields(exe, n_cu):
    out = _geometry(exe, [(n_cu, n, nb) for n in N_COUNTS for nb in N_BYTES])
    for g in out:
        _check(g)
    if n_cu == 256:      # the anchors of the GPU cases (tests/test_gpu_ctdefer.py)
        shape = {g["n_counts"]: (g["n_bins"], g["region"]) for g in out}
        assert shape[8_388_608] == (256, 32768) and shape[8_388_609] == (512, 16385) and shape[58_720_257] == (2048, 28673)
        assert shape[67_108_864] == (2048, 32768) and shape[300] == (2, 256) and shape[5_000] == (20, 256)
        assert shape[25_600_000] == (1024, 25000)


def test_tables_and_devices_not_served(exe):
    """One counter more than 2 048 regions of 32 768 hold, no counters, no CU -- and one CU: n_wg = 0 divided by zero."""
    out = _geometry(exe, [(256, 67_108_865, 0), (2, 67_108_865, 1 << 30), (256, 0, 0), (0, 300, 0), (1, 300, 0), (1, 1_800_000, 1 << 30), (1, 67_108_864, 0)])
    assert [g["bytes"] for g in out] == [0] * len(out)
    for g in _geometry(exe, [(3, n, 0) for n in N_COUNTS]):      # an odd count of CUs: the even number below
        _check(g)
        assert g["n_wg"] == 2


@pytest.mark.parametrize("cap_knob,room_knob", [("-1", None), ("-40000", "-3"), ("0", "0"), ("40000", None), (None, "7"), (None, "500"), ("40000", "99999999"),
                                                ("99999999999999", "99999999999999"), ("9223372036854775807", "9223372036854775807"), ("junk", "junk")])
def test_test_knobs_are_clamped(exe, cap_knob, room_knob):
    """VGMI_CT_DEFER_CAP / VGMI_CT_DEFER_ROOM (a record buffer / rooms that fill up): whatever they say, CTD_CHUNK <= cap <= 0xC0000000
    and 1 <= room <= cap."""
    env = {}
    if cap_knob is not None:
        env["VGMI_CT_DEFER_CAP"] = cap_knob
    if room_knob is not None:
        env["VGMI_CT_DEFER_ROOM"] = room_knob
    out = _geometry(exe, [(n_cu, n, 45_000_000) for n_cu in (256, 2) for n in (300, 1_800_000, 67_108_864)], env=env)
    for g in out:
        _check(g, knobs=True)
        if cap_knob == "40000":
            assert g["cap"] == 40448      # rounded up to whole chunks, and one more
        if cap_knob in ("-1", "-40000", "0", "junk"):
            assert g["cap"] == CTD_CHUNK
        if room_knob in ("7", "500"):
            assert g["room"] == int(room_knob) + 1
        if room_knob in ("-3",):
            assert g["room"] == 1
