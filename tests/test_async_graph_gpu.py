"""Every device-pointer (_async) entry point of include/tfhe_mi355.h replayed from a captured hipGraph.

The header promises that an _async call "can be captured into a hipGraph (no allocation or synchronisation
inside)" and holds no per-context mutable state.  tests/test_async_guards_gpu.py pins what each call computes and
where it writes when it runs eagerly (the host-pointer twin, the oracle, the guard bands); this file takes the
same case table -- tests/test_lwe_ingress_gpu.py adds its cases at import -- and runs every case from a graph.
None of what follows changes an eager result, so only a replay shows it: a host value or a context-owned pointer
baked in at capture time, device data read on the host between launches, a context buffer reallocated under a
graph, a memset or flag reset on the host side of a launcher, a replay that leans on what the one before left in
the scratch (the quad flags, the persistent grid's ticket, the keyswitch digit planes).

Per case, on an arena built as the guards runner builds it (every region at 16 modulo 256, the scratch of exactly
the queried size, none where the query is 0), comparisons by byte equality throughout:

  1. eager A: one call outside any capture (the warm-up), under the kernel timer: the kernel families of the
     case ran; outA;
  2. eager B: the primary ciphertext input XORed in place with a seeded random stream: outB != outA; restored;
  3. capture: guards, output and scratch refilled from another stream, in-place operands restored; one call
     captured with torch.cuda.graph on a side stream with the kernel timer on (every = 1): no byte of the arena
     changed (the capture ran nothing), and the timer holds no entry;
  4. replay 1: outA, arena.check() == [];
  5. replay 2, after another refill: outA (nothing depends on the output or scratch of the replay before);
  6. replay 3, the change of step 2 made through the same device buffers: outB (no snapshot of the inputs lives
     in the graph);
  7. graph and arena stay alive until the engine's last case; then every kept graph of the engine replays once
     more, in reverse order, from refilled arenas, to its outA: in between the context has served eager and
     captured calls of other counts, kernel forms and scratch sizes.  Then the graphs are released and the
     engine closed.

The device is synchronised before and after every replay: no two graphs, and no graph and eager call, are ever
in flight together (the quad CMUX cases need the device to themselves, as in the guards file).  Index and opcode
arrays, Fourier GGSW lists and key regions never change.  No TFHE_MI355_* variable is set: `count` selects the
kernel form.

The entry points of NOT_CAPTURABLE wait for their stream before they return; the header says so.  They are not
replayed: called on a capturing stream they fail (rc 1, a message naming stream capture) before they lock or
enqueue anything, so the caller's capture stays valid -- their cases check exactly that.

This file keeps its own engines and leaves the guards runner's ENGINES / _LAST_OF_ENGINE alone; it passes alone
and in a run over tests/.
"""
from types import SimpleNamespace as NS

import numpy as np
import pytest

import test_async_guards_gpu as G
import test_lwe_ingress_gpu  # noqa: F401  (registers the ingress cases in G.CASES)
from guarded_arena import splitmix64

pytestmark = pytest.mark.gpu

_WAITS = ("keys uploaded through the _async/device forms are complete when the upload call returns "
          "(it waits for its stream), so any later call on any stream sees the whole key")
# entry points that cannot be captured: {name: the header sentence that says the call waits}
NOT_CAPTURABLE = {
    G.P + "bootstrap_key_convert_async": _WAITS,
    G.P + "keyswitch_key_upload_async": _WAITS,
}

# read-only regions that are no ciphertext input: index and opcode arrays, Fourier GGSW lists, seeds, keys
NOT_CIPHERTEXT = {"lut_indexes", "indexes", "ops", "fourier", "seeds", "bsk", "ksk"}

# the ordinary call captured next to a refused upload: KS and PBS, so its replay reads both resident keys
ORDINARY = "pbsks-2048-1"

# arena streams: 1 at allocation (eager A and B), then one per refill; the mask of the changed input
SEED_CAPTURE, SEED_REPLAY, SEED_LAST, SEED_MASK = 3, 4, 5, 1009

_first = {}
for _c in G.CASES:
    _first.setdefault(_c.engine, len(_first))
CASES = sorted(G.CASES, key=lambda c: _first[c.engine])  # stable: engine by engine


def capturable(c):
    return not any(e in NOT_CAPTURABLE for e in c.entries)


def replayed_entry_points():
    """{entry point: ids of the cases this file replays from a graph}"""
    out = {}
    for c in CASES:
        if capturable(c):
            for e in c.entries:
                out.setdefault(e, []).append(c.id)
    return out


_LAST = {c.engine: c.id for c in CASES if capturable(c)}
_OPEN = {}  # engine key -> NS(E, kept: the runs whose graphs are alive)


def _holder(key, orc):
    if key not in _OPEN:
        _OPEN[key] = NS(E=G.FACTORIES[key](orc), kept=[])
    return _OPEN[key]


def _primary(spec):
    name = getattr(spec, "primary", None)
    if name is None:
        name = next(r.name for r in spec.regions if not r.writable and r.name not in NOT_CIPHERTEXT)
    assert name not in NOT_CIPHERTEXT and name != spec.scratch[0]
    return next(r for r in spec.regions if r.name == name)


def _load(run, changed):
    """the inputs as declared (in-place operands restored), or with the primary input XOR the mask"""
    run.arena.restore()
    if run.primary.writable:  # an in-place operand: just restored
        run.is_changed = False
    if run.is_changed != changed:
        run.views[run.primary.name].bitwise_xor_(run.mask)
        run.is_changed = changed


def _output(run):
    import torch

    torch.cuda.synchronize()
    return run.views[run.spec.out].clone()


def _same(got, want, row, what):
    import torch

    if not torch.equal(got, want):
        raise AssertionError(what + ": " + G._first_difference(got.cpu().numpy(), want.cpu().numpy(), row))


def _replay(run):
    import torch

    torch.cuda.synchronize()
    run.graph.replay()
    torch.cuda.synchronize()


def _eager(cid, E, spec):
    """steps 1 and 2: the arena of the case, outA (under the kernel timer) and outB"""
    import torch

    arena, views = G.build_arena(spec)
    primary = _primary(spec)
    words = (primary.nbytes + 7) // 8
    mask = splitmix64(0, words, SEED_MASK, arena.device).view(torch.uint8)[:primary.nbytes]
    run = NS(id=cid, eng=E.eng, spec=spec, arena=arena, views=views, primary=primary, mask=mask, is_changed=False,
             graph=None, outA=None, outB=None)
    eng = E.eng
    eng.kernel_timing(1)
    spec.call(views)
    run.outA = _output(run)
    ran = set(eng.kernel_times())
    eng.kernel_timing(0)
    if spec.kernels is not None:
        assert spec.kernels <= ran, f"expected kernel families {spec.kernels}, ran {ran}"
    assert arena.check() == []
    _load(run, True)
    spec.call(views)
    run.outB = _output(run)
    assert not torch.equal(run.outB, run.outA), f"the output does not follow region {primary.name}"
    _load(run, False)
    assert arena.check() == [], "the changed input was not put back"
    return run


def _capture(run, extra=None):
    """step 3: one call captured on a side stream under the kernel timer; extra(): more inside the same capture"""
    import torch

    eng, arena = run.eng, run.arena
    arena.refill(SEED_CAPTURE)
    _load(run, False)
    torch.cuda.synchronize()
    before = arena.buf.clone()
    graph = torch.cuda.CUDAGraph()
    eng.kernel_timing(1)
    try:
        with torch.cuda.graph(graph):
            run.spec.call(run.views)
            if extra is not None:
                extra()
        torch.cuda.synchronize()
        timed = eng.kernel_times()
    finally:
        eng.kernel_timing(0)
    out = run.views[run.spec.out]
    at = out.data_ptr() - arena.buf.data_ptr()
    _same(out, before[at:at + out.numel()], run.spec.out_row, "the capture wrote the output")
    assert torch.equal(arena.buf, before), "the capture changed the arena: something ran"
    assert arena.check() == []
    assert timed == {}, f"kernels were timed while the stream was being captured: {timed}"
    run.graph = graph


def _replays(run):
    """steps 4 to 6"""
    row = run.spec.out_row
    _replay(run)
    _same(_output(run), run.outA, row, "replay 1 differs from the eager call")
    assert run.arena.check() == [], f"replay 1 wrote outside its output and scratch: {run.arena.check()}"
    run.arena.refill(SEED_REPLAY)
    _load(run, False)
    _replay(run)
    _same(_output(run), run.outA, row, "replay 2 depends on what the output or scratch held before")
    assert run.arena.check() == [], f"replay 2 wrote outside its output and scratch: {run.arena.check()}"
    _load(run, True)
    _replay(run)
    _same(_output(run), run.outB, row, f"replay 3 does not follow region {run.primary.name}")
    _load(run, False)
    assert run.arena.check() == []


def _finish(key):
    """step 7: every kept graph of the engine once more, newest first; then the graphs go, then the engine"""
    import torch

    h = _OPEN.pop(key)
    errors = []
    try:
        for run in reversed(h.kept):
            try:
                run.arena.refill(SEED_LAST)
                _load(run, False)
                _replay(run)
                _same(_output(run), run.outA, run.spec.out_row, "the last replay differs from the eager call")
                assert run.arena.check() == [], f"the last replay wrote outside: {run.arena.check()}"
            except AssertionError as e:
                errors.append(f"{run.id}: {e}")
    finally:
        torch.cuda.synchronize()
        for run in h.kept:
            run.graph = None
        h.kept.clear()
        h.E.eng.close()
    assert not errors, errors


def _refused(orc, c):
    """a NOT_CAPTURABLE form called inside a capture: EngineError, and the capture, the graph and the resident
    keys are as if it had not been called"""
    import torch

    from tfhe_mi355 import EngineError

    (entry,) = c.entries
    E = G.FACTORIES["c2048"](orc)  # holds both keys; this test's own
    try:
        eng = E.eng
        keys = G._snapshot(E)
        source = {G.P + "bootstrap_key_convert_async": E.bsk, G.P + "keyswitch_key_upload_async": E.ksk}[entry]
        d_source = torch.from_numpy(source.view(np.int64)).cuda()

        def upload():
            if entry == G.P + "bootstrap_key_convert_async":
                eng.convert_bootstrap_key_device(d_source, source.size)
            else:
                eng.upload_keyswitch_key_device(d_source, source.size)

        def refused():
            with pytest.raises(EngineError, match="stream capture"):
                upload()

        spec = next(x for x in G.CASES if x.id == ORDINARY).build(E, orc)
        run = _eager(ORDINARY, E, spec)
        _capture(run, extra=refused)  # the block ends without error
        _replay(run)
        _same(_output(run), run.outA, spec.out_row, "the graph next to the refused upload differs from the eager call")
        assert run.arena.check() == []
        after = G._snapshot(E)
        assert set(after) == set(keys) == {"fourier", "ksk"}
        for part in keys:
            assert np.array_equal(after[part], keys[part]), f"the refused upload changed the resident {part} key"
        upload()  # outside a capture the form serves as before, and the same words give the same key
        after = G._snapshot(E)
        for part in keys:
            assert np.array_equal(after[part], keys[part]), part
        _replay(run)
        _same(_output(run), run.outA, spec.out_row, "the graph differs after the eager upload of the same key")
        run.graph = None
    finally:
        torch.cuda.synchronize()
        E.eng.close()


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.id)
def test_captured_call(orc, c):
    if not capturable(c):
        assert set(c.entries) <= set(NOT_CAPTURABLE)
        _refused(orc, c)
        return
    h = _holder(c.engine, orc)
    try:
        spec = c.build(h.E, orc)
        assert spec.out is not None, "a case without an output region is a key upload: it belongs to NOT_CAPTURABLE"
        run = _eager(c.id, h.E, spec)
        _capture(run)
        h.kept.append(run)
        _replays(run)
    finally:
        if _LAST[c.engine] == c.id:
            _finish(c.engine)


def test_engines_left_open_replay_and_close():
    """engines whose last case was deselected: the same last replays, and the close"""
    errors = []
    for key in list(_OPEN):
        try:
            _finish(key)
        except AssertionError as e:
            errors.append(str(e))
    assert not errors, errors
