"""CPU tests of tests/guarded_arena.py itself, and the completeness check of the guarded case table
(tests/test_async_guards_gpu.py) against the header: every *_async entry point of
include/tfhe_mi355.h has a guarded case or a stated reason for having none."""
import os
import re

import numpy as np
import pytest
import torch

from guarded_arena import MIN_GUARD, GuardedArena, splitmix64, splitmix64_int

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _arena(seed=1):
    """lwe (read-only u64 rows, align 16), idx (read-only, align 4), out (writable, align 8), a LUT whose
    row is wider than half the minimal band, scratch (writable)"""
    rng = np.random.default_rng(3)
    a = GuardedArena("cpu", seed)
    a.region("lwe", 5 * 24, data=rng.integers(0, 2 ** 64, 15, dtype=np.uint64), row=24)
    a.region("idx", 5 * 4, align=4, data=np.arange(5, dtype=np.uint32), row=4)
    a.region("out", 5 * 40, align=8, writable=True, row=40)
    a.region("lut", 2 * 40960, data=rng.integers(0, 2 ** 64, 2 * 5120, dtype=np.uint64), row=40960)
    a.region("scratch", 256, writable=True)
    return a.allocate()


def test_region_addresses_have_the_stated_residues():
    a = _arena()
    assert a.buf.data_ptr() % 256 == 0
    for r, align in zip(a.regions, (16, 4, 8, 16, 16)):
        assert r.align == align
        assert r.view.data_ptr() % 256 == align, (r.name, r.view.data_ptr() % 256)
        assert r.view.data_ptr() % (2 * align) != 0  # no more aligned than stated
        assert r.view.is_contiguous() and r.view.numel() == r.nbytes
        assert r.view.data_ptr() == a.buf.data_ptr() + r.offset
        assert a.view(r.name).data_ptr() == r.view.data_ptr()


def test_bands_surround_every_region_and_have_the_stated_width():
    a = _arena()
    kinds = [s[3] for s in a.segments]
    assert kinds == ["guard", "ro", "guard", "ro", "guard", "rw", "guard", "ro", "guard", "rw", "guard"]
    assert a.segments[0][1] == 0 and a.segments[-1][2] == a.buf.numel()
    for (_, _, e0, _), (_, s1, _, _) in zip(a.segments, a.segments[1:]):
        assert e0 == s1  # the segments tile the arena
    rows = [0] + [r.row for r in a.regions] + [0]
    guards = [s for s in a.segments if s[3] == "guard"]
    assert len(guards) == len(a.regions) + 1
    for i, (name, s, e, _) in enumerate(guards):
        need = max(MIN_GUARD, 2 * max(rows[i], rows[i + 1]))
        assert e - s >= need, (name, e - s, need)
    # the bands beside the 40960-byte LUT rows are row-sized, not the 64 KiB minimum
    assert guards[3][2] - guards[3][1] >= 81920 and guards[4][2] - guards[4][1] >= 81920


def test_fill_is_the_seeded_position_dependent_stream_and_regions_hold_their_data():
    a = _arena(seed=5)
    words = a.buf.view(torch.int64)
    for w in (0, 1, 7, words.numel() - 1):  # inside the first and the last band
        assert int(words[w]) & (2 ** 64 - 1) == splitmix64_int(w, 5)
    got = splitmix64(11, 4, 9, "cpu")
    assert [int(x) & (2 ** 64 - 1) for x in got] == [splitmix64_int(11 + i, 9) for i in range(4)]
    assert len({splitmix64_int(i, 5) for i in range(1000)}) == 1000
    assert np.array_equal(a.view("idx").numpy().view(np.uint32), np.arange(5, dtype=np.uint32))
    out = a.regions[2]
    w0 = (out.offset + 7) // 8  # the writable region holds the stream as well
    assert int(words[w0]) & (2 ** 64 - 1) == splitmix64_int(w0, 5)
    assert a.check() == []


def test_one_byte_in_each_band_in_turn_is_reported_exactly():
    a = _arena()
    for name, s, e, kind in a.segments:
        if kind != "guard":
            continue
        for off in (0, (e - s) // 2, e - s - 1):
            old = int(a.buf[s + off])
            a.buf[s + off] = old ^ 0x5A
            assert a.check() == [(name, off, off)]
            a.buf[s + off] = old
            assert a.check() == []


def test_one_byte_in_a_read_only_region_is_reported_exactly():
    a = _arena()
    for r in a.regions:
        if r.writable:
            continue
        for off in (0, r.nbytes - 1):
            r.view[off] ^= 1
            assert a.check() == [(r.name, off, off)]
            r.view[off] ^= 1
            assert a.check() == []


def test_the_bytes_next_to_a_writable_region_are_guarded_and_its_inside_is_not():
    a = _arena()
    segs = a.segments
    for i, (name, s, e, kind) in enumerate(segs):
        if kind != "rw":
            continue
        a.buf[s:e] = 0  # the whole writable region
        a.buf[s] = 0xFF
        a.buf[e - 1] = 0xFF
        assert a.check() == []
        before, after = segs[i - 1], segs[i + 1]
        a.buf[s - 1] ^= 0x80
        assert a.check() == [(before[0], before[2] - before[1] - 1, before[2] - before[1] - 1)]
        a.buf[s - 1] ^= 0x80
        a.buf[e] ^= 0x80
        assert a.check() == [(after[0], 0, 0)]
        a.buf[e] ^= 0x80
        assert a.check() == []


def test_first_and_last_changed_offsets_and_several_segments():
    a = _arena()
    g = a.segments[4]  # the band before `out`
    a.buf[g[1] + 10] ^= 1
    a.buf[g[1] + 4000] ^= 1
    a.view("lwe")[17] ^= 1
    assert a.check() == [("lwe", 17, 17), (g[0], 10, 4000)]


def test_refill_changes_guards_and_writable_regions_only():
    a = _arena(seed=1)
    before = a.buf.clone()
    with pytest.raises(ValueError):
        a.refill(1)
    a.refill(2)
    assert a.check() == []
    for name, s, e, kind in a.segments:
        same = torch.equal(a.buf[s:e], before[s:e])
        assert same == (kind == "ro"), name
        if kind != "ro":  # another stream: (almost) every word differs
            w = (a.buf[s:e] != before[s:e]).float().mean()
            assert w > 0.9, (name, float(w))
    # eight bytes of the old stream in a band are now a change
    g = a.segments[0]
    a.buf[g[1] + 8:g[1] + 16] = before[g[1] + 8:g[1] + 16]
    got = a.check()
    assert len(got) == 1 and got[0][0] == g[0] and 8 <= got[0][1] <= got[0][2] <= 15
    a.refill(3)
    assert a.check() == []


def test_declaration_errors():
    a = GuardedArena("cpu")
    with pytest.raises(ValueError):
        a.region("x", 8)  # read-only without data
    with pytest.raises(ValueError):
        a.region("x", 8, data=np.zeros(2, dtype=np.uint64))  # 16 bytes of data for 8
    with pytest.raises(ValueError):
        a.region("x", 8, align=24, writable=True)
    a.region("x", 8, writable=True)
    with pytest.raises(ValueError):
        a.region("x", 8, writable=True)
    a.allocate()
    with pytest.raises(RuntimeError):
        a.region("y", 8, writable=True)


# ---- completeness: every _async entry point of the header has a guarded case ------------------------

def _header_async_entry_points():
    with open(os.path.join(ROOT, "include", "tfhe_mi355.h")) as f:
        text = f.read()
    return sorted(set(re.findall(r"^int (tfhe_mi355_\w+_async)\(", text, flags=re.M)))


def test_every_async_entry_point_has_a_guarded_case_or_a_reason():
    import test_async_guards_gpu as G

    names = _header_async_entry_points()
    assert len(names) >= 30 and "tfhe_mi355_programmable_bootstrap_async" in names, names
    covered = G.covered_entry_points()
    for n in names:
        assert (n in covered) != (n in G.EXCLUDED), f"{n}: needs a guarded case or an exclusion (not both)"
    for n in list(covered) + list(G.EXCLUDED):
        assert n in names, f"{n} is not an _async entry point of the header"
    for n, why in G.EXCLUDED.items():
        assert isinstance(why, str) and len(why) > 20, n


def test_every_guarded_entry_point_is_replayed_from_a_graph_or_documented_as_waiting():
    """tests/test_async_graph_gpu.py replays the guarded cases (the ingress cases among them: it imports both case
    modules) from captured graphs: every entry point with a guarded case has a replayed one, or stands in
    NOT_CAPTURABLE under a sentence of the header that says the call waits -- never both."""
    import test_async_graph_gpu as R
    import test_async_guards_gpu as G

    covered = G.covered_entry_points()
    assert "tfhe_mi355_lwe_expand_async" in covered and "tfhe_mi355_apply_from_async" in covered
    replayed = R.replayed_entry_points()
    assert len({c.id for c in R.CASES}) == len(R.CASES) == len(G.CASES)
    for n in covered:
        assert (n in replayed) != (n in R.NOT_CAPTURABLE), f"{n}: needs a replayed case or a header sentence (not both)"
    for n in list(replayed) + list(R.NOT_CAPTURABLE):
        assert n in covered, f"{n} has no guarded case"
    with open(os.path.join(ROOT, "include", "tfhe_mi355.h")) as f:
        header = " ".join(f.read().replace("*", " ").split())
    for n, sentence in R.NOT_CAPTURABLE.items():
        assert "waits" in sentence and " ".join(sentence.split()) in header, f"{n}: the header does not say so"
        at = header.index("refuse a capturing stream")  # the capture paragraph names the forms that do
        assert n in header[max(at - 400, 0):at], n
