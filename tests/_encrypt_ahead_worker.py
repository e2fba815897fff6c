"""The ahead path of the seed-mode single-dealer encrypt (pvw_encrypt_device on a stream where the MAC of the previous such call
is still outstanding: the prologue runs on the workspace's side stream into a ring of (r-hat, e_small) sets, the calling thread
waits for it, and the MAC is enqueued with nothing in front of it), with torch tensors as device memory and torch streams.  The
stream is made busy with torch.cuda._sleep in front of the calls, so every call after the first finds its predecessor's MAC
outstanding.  The yardstick of every result is the same call made alone on an idle stream (which stays in order), and for some
of them the C oracle.  The profiling scope `prologue_ahead` tells which path a call took.

torch is imported FIRST so both libraries share one HIP runtime.  Spawned by tests/test_encrypt_ahead.py:
`python _encrypt_ahead_worker.py <case> [geometry]` prints AHEAD_OK on success."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import torch  # noqa: F401  (must precede pvw_rs_amd in this process)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import pvw_model as M  # noqa: E402
import pvw_oracle as O  # noqa: E402
import pvw_rs_amd as P  # noqa: E402
from pvw_rs_amd import _ffi, api  # noqa: E402
from pvw_rs_amd.workloads import REFERENCE_128_MODULI  # noqa: E402

DEV = torch.device("cuda", 0)
S = bytes(range(101, 133))
# long enough to outlast the host side of every sequence below (a dozen calls, each of which may poll for a millisecond) at
# any clock the counter of _sleep may run at
SLEEP_CYCLES = 50_000_000
CALLS = 12                              # more than the ring has sets (2, and 16 at the most): the sequence wraps

# name: (n, k, l, moduli, packed width the MAC streams at)
GEOMETRIES = {
    "A": (48, 256, 8, M.bench_moduli(3), 61),              # mac_rows_packed61
    "B": (20, 64, 16, REFERENCE_128_MODULI[:2], 56),       # mac_rows_packedw
    "C": (12, 24, 8, M.bench_moduli(2), 0),                # mac_rows (k is no multiple of 64: no packed copy)
}


def ptr(t):
    return C.c_void_p(t.data_ptr())


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def seed_of(i):
    return bytes([(31 * i + 7 * j + 1) & 0xFF for j in range(32)])


def scalars_of(n, i):
    return [(i * 1000003 + 7919 * j + (j << 33) + 1) % (1 << 64) for j in range(n)]


def dev_u64(vals):
    return torch.from_numpy(np.ascontiguousarray(np.array(vals, dtype=np.uint64)).view(np.int64)).to(DEV)


class Setup:
    def __init__(self, n, k, l, moduli):
        self.n, self.k, self.l, self.L, self.moduli = n, k, l, len(moduli), moduli
        self.p = P.PvwParametersBuilder().set_parties(n).set_dimension(k).set_l(l).set_moduli(moduli).build()
        self.crs = P.PvwCrs.new_deterministic(self.p, S)
        self.gpk = P.GlobalPublicKey.new(self.crs)
        self.gpk.fill_uniform(S)
        self.lib = _ffi.lib()

    def outputs(self):
        return (torch.zeros((self.k, self.L, self.l), dtype=torch.int64, device=DEV),
                torch.zeros((self.n, self.L, self.l), dtype=torch.int64, device=DEV))

    def seed_call(self, sc, seed, c1, c2, s):
        rnd, _ = api._randomness(self.p, seed, None, None, None)
        api._check(self.lib.pvw_encrypt_device(self.p._h, ptr(sc), self.n, C.byref(rnd), ptr(c1), ptr(c2), P.REPR_NTT,
                                               C.c_void_p(s.cuda_stream)), self.lib)

    def rs_call(self, sc, st, c1, c2, s):
        api._check(self.lib.pvw_encrypt_rs_device(self.p._h, ptr(sc), self.n, st._h, ptr(c1), ptr(c2), P.REPR_NTT,
                                                  C.c_void_p(s.cuda_stream)), self.lib)

    def explicit(self, seed):
        """r, e1, e2 of `seed` as device arrays, and the pvw_randomness_t that points at them"""
        arrs = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(DEV) for a in self.sampled(seed)]
        rnd = _ffi.pvw_randomness_t()
        rnd.mode = _ffi.RND_EXPLICIT
        rnd.r, rnd.e1, rnd.e2 = (a.data_ptr() for a in arrs)
        return rnd, arrs

    def explicit_call(self, sc, rnd, c1, c2, s):
        api._check(self.lib.pvw_encrypt_device(self.p._h, ptr(sc), self.n, C.byref(rnd), ptr(c1), ptr(c2), P.REPR_NTT,
                                               C.c_void_p(s.cuda_stream)), self.lib)

    def sampled(self, seed):
        return (O.sample_cbd(seed, M.DOM_R, 0, self.k, self.l, 0.5), O.sample_uniform(seed, M.DOM_E1, 0, self.k, self.l, 100),
                O.sample_uniform(seed, M.DOM_E2, 0, self.n, self.l, 200))

    def alone(self, vals, seed):
        """the same seed-mode call made alone on an idle stream: (c1, c2) as uint64 arrays"""
        torch.cuda.synchronize()
        s = torch.cuda.Stream(device=DEV)
        sc, (c1, c2) = dev_u64(vals), self.outputs()
        torch.cuda.synchronize()
        self.seed_call(sc, seed, c1, c2, s)
        torch.cuda.synchronize()
        return u64(c1), u64(c2)

    def oracle(self, vals, seed):
        orc = O.Oracle(self.moduli, self.l)
        r, e1, e2 = self.sampled(seed)
        return orc.encrypt(self.crs.matrix(P.REPR_NTT), self.gpk.matrix(repr=P.REPR_NTT), self.p.gadget_polynomial(P.REPR_NTT),
                           np.array(vals, dtype=np.uint64), r, e1, e2)

    def launches(self, name):
        return self.p.kernel_time(name)[1]


def busy(s):
    with torch.cuda.stream(s):
        torch.cuda._sleep(SLEEP_CYCLES)


def short_sleep(s, us):
    """the stream asleep for about `us` microseconds: _sleep counts a clock whose rate is measured here, once"""
    global _CYCLES_PER_US
    if _CYCLES_PER_US is None:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        torch.cuda._sleep(2_000_000)
        b.record()
        torch.cuda.synchronize()
        _CYCLES_PER_US = 2_000_000 / (a.elapsed_time(b) * 1000.0)
    with torch.cuda.stream(s):
        torch.cuda._sleep(max(1, int(us * _CYCLES_PER_US)))


_CYCLES_PER_US = None


def exact(geometry):
    """CALLS seed-mode calls back to back on one busy stream, no sync between them, distinct seeds, scalars and output buffers:
    each equals the same call made alone; calls 1 and 9 also equal the C oracle; the profiling scopes say the ahead path ran,
    and every call made exactly one prologue.  Behind the long sleep every guard the side stream waits for stays outstanding,
    so from the ring's first wrap on the calls run out of their poll and order the MAC by a wait packet.  A second burst of the
    same calls follows behind a sleep of 0.6 ms, shorter than the poll's bound: there the guard wait of the wrap ends while the
    calling thread still polls, and the MAC goes out with nothing in front of it, as in back-to-back use."""
    n, k, l, moduli, width = GEOMETRIES[geometry]
    g = Setup(n, k, l, moduli)
    s = torch.cuda.Stream(device=DEV)
    vals = [scalars_of(n, i) for i in range(CALLS)]
    scs = [dev_u64(v) for v in vals]
    outs = [g.outputs() for _ in range(CALLS)]
    # the first call of a context builds the packed copies and waits for them: made here, on an idle stream
    g.seed_call(scs[0], seed_of(100), *g.outputs(), s)
    torch.cuda.synchronize()
    assert g.p.packed_active() == width, g.p.packed_active()
    g.p.set_profiling(True)
    g.p.reset_profiling()
    busy(s)
    for i in range(CALLS):
        g.seed_call(scs[i], seed_of(i), outs[i][0], outs[i][1], s)
    torch.cuda.synchronize()
    ahead, in_order, macs = g.launches("prologue_ahead"), g.launches("prologue"), g.launches("mac_rows")
    g.p.set_profiling(False)
    print(f"geometry {geometry}: prologue_ahead {ahead}, prologue {in_order}, mac_rows {macs}", flush=True)
    # the first call has no MAC in front of it and stays in order; the others go ahead unless the GPU caught up with the host
    assert ahead >= 1 and in_order >= 1 and ahead + in_order == CALLS and macs == CALLS, (ahead, in_order, macs)
    want = [g.alone(vals[i], seed_of(i)) for i in range(CALLS)]
    for i in range(CALLS):
        assert np.array_equal(u64(outs[i][0]), want[i][0]), f"geometry {geometry} call {i}: c1"
        assert np.array_equal(u64(outs[i][1]), want[i][1]), f"geometry {geometry} call {i}: c2"
    again = [g.outputs() for _ in range(CALLS)]
    torch.cuda.synchronize()
    g.p.set_profiling(True)
    g.p.reset_profiling()
    short_sleep(s, 600)
    for i in range(CALLS):
        g.seed_call(scs[i], seed_of(i), again[i][0], again[i][1], s)
    torch.cuda.synchronize()
    ahead, in_order = g.launches("prologue_ahead"), g.launches("prologue")
    g.p.set_profiling(False)
    print(f"geometry {geometry}, short sleep: prologue_ahead {ahead}, prologue {in_order}", flush=True)
    assert ahead + in_order == CALLS, (ahead, in_order)      # which calls go ahead depends on when the sleep ends
    for i in range(CALLS):
        assert np.array_equal(u64(again[i][0]), want[i][0]), f"geometry {geometry} short sleep, call {i}: c1"
        assert np.array_equal(u64(again[i][1]), want[i][1]), f"geometry {geometry} short sleep, call {i}: c2"
    for i in (1, 9):
        o1, o2 = g.oracle(vals[i], seed_of(i))
        assert np.array_equal(u64(outs[i][0]), o1) and np.array_equal(u64(outs[i][1]), o2), f"geometry {geometry} call {i}: oracle"
    assert not np.array_equal(u64(outs[0][0]), u64(outs[8][0]))      # two users of one set, whatever the ring's size


def ordered():
    """What the caller queued on its stream still orders the MAC: one scalars tensor rewritten by a torch kernel between the
    calls, one pair of output buffers copied aside by stream-ordered copies."""
    n, k, l, moduli, _ = GEOMETRIES["A"]
    g = Setup(n, k, l, moduli)
    s = torch.cuda.Stream(device=DEV)
    vals = [scalars_of(n, 50 + i) for i in range(CALLS)]
    srcs = [dev_u64(v) for v in vals]
    sc = torch.zeros(n, dtype=torch.int64, device=DEV)
    c1, c2 = g.outputs()
    kept = [g.outputs() for _ in range(CALLS)]
    g.seed_call(srcs[0], seed_of(100), *g.outputs(), s)
    torch.cuda.synchronize()
    g.p.set_profiling(True)
    g.p.reset_profiling()
    busy(s)
    with torch.cuda.stream(s):
        for i in range(CALLS):
            torch.add(srcs[i], 0, out=sc)
            g.seed_call(sc, seed_of(50 + i), c1, c2, s)
            kept[i][0].copy_(c1)
            kept[i][1].copy_(c2)
    torch.cuda.synchronize()
    ahead = g.launches("prologue_ahead")
    g.p.set_profiling(False)
    assert ahead >= 1, ahead
    for i in range(CALLS):
        w1, w2 = g.alone(vals[i], seed_of(50 + i))
        assert np.array_equal(u64(kept[i][0]), w1) and np.array_equal(u64(kept[i][1]), w2), f"call {i}"


def paths():
    """`prologue_ahead` counts nothing for a single call on an idle stream, an _rs call, explicit randomness, and l = 32 (full
    addends) -- the last three behind a seed-mode call on a busy stream, where a second seed-mode call of geometry A does take
    the ahead path.  A captured call: the capture succeeds and its replay equals the eager result.  That is the evidence for it;
    the count is none (profiling is off around the capture, whose event pairs are not for a graph, and the stream is idle when
    the capture begins) -- what keeps a captured call in order is that the ahead path's queries are never made of a capturing
    stream, and a query there would end the capture with an error."""
    n, k, l, moduli, _ = GEOMETRIES["A"]
    g = Setup(n, k, l, moduli)
    s = torch.cuda.Stream(device=DEV)
    vals = scalars_of(n, 7)
    sc = dev_u64(vals)
    assert g.p.prepare(P.PREPARE_PACKED, s.cuda_stream) > 0 and g.p.packed_active() == 61
    torch.cuda.synchronize()
    want = g.alone(vals, seed_of(7))
    g.p.set_profiling(True)

    def counted(what, expect_ahead, expect_in_order):
        torch.cuda.synchronize()
        got = (g.launches("prologue_ahead"), g.launches("prologue"))
        print(what, got, flush=True)
        assert got == (expect_ahead, expect_in_order), (what, got)
        g.p.reset_profiling()

    g.p.reset_profiling()
    d1, d2 = g.outputs()

    def busy_with_a_seed_call():
        """the stream asleep with one seed-mode call queued behind that (in order: nothing of its kind is in front of it)"""
        busy(s)
        g.seed_call(sc, seed_of(8), d1, d2, s)

    # the control: seed mode, compact addends, the previous call's MAC outstanding
    c1, c2 = g.outputs()
    busy_with_a_seed_call()
    g.seed_call(sc, seed_of(7), c1, c2, s)
    counted("seed call behind a seed call", 1, 1)
    assert np.array_equal(u64(c1), want[0]) and np.array_equal(u64(c2), want[1])
    # idle stream
    c1, c2 = g.outputs()
    torch.cuda.synchronize()
    g.seed_call(sc, seed_of(7), c1, c2, s)
    counted("idle seed call", 0, 1)
    assert np.array_equal(u64(c1), want[0]) and np.array_equal(u64(c2), want[1])
    # _rs on a busy stream
    with P.DeviceRandomness(g.p, S, 40) as st:
        c1, c2 = g.outputs()
        busy_with_a_seed_call()
        g.rs_call(sc, st, c1, c2, s)
        counted("_rs call behind a seed call", 0, 2)
        w = g.alone(vals, P.DeviceRandomness.call_seed(S, 40))
        assert np.array_equal(u64(c1), w[0]) and np.array_equal(u64(c2), w[1])
        g.p.reset_profiling()
    # explicit randomness on a busy stream
    rnd, keep = g.explicit(seed_of(7))
    c1, c2 = g.outputs()
    busy_with_a_seed_call()
    g.explicit_call(sc, rnd, c1, c2, s)
    counted("explicit call behind a seed call", 0, 2)
    assert np.array_equal(u64(c1), want[0]) and np.array_equal(u64(c2), want[1])
    del keep
    # under capture (profiling off: its event pairs are not for a graph)
    g.p.set_profiling(False)
    c1, c2 = g.outputs()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    rnd7, _ = api._randomness(g.p, seed_of(7), None, None, None)
    with torch.cuda.graph(graph, stream=s):
        rc = g.lib.pvw_encrypt_device(g.p._h, ptr(sc), n, C.byref(rnd7), ptr(c1), ptr(c2), P.REPR_NTT,
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))
    api._check(rc, g.lib)
    torch.cuda.synchronize()
    assert not u64(c1).any()                                 # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(u64(c1), want[0]) and np.array_equal(u64(c2), want[1]), "graph replay"
    del graph
    # l = 32: the addends are full polynomials, which the prologue adds the scalars to
    g32 = Setup(8, 16, 32, M.bench_moduli(2))
    s32 = torch.cuda.Stream(device=DEV)
    v32 = scalars_of(8, 3)
    sc32 = dev_u64(v32)
    g32.seed_call(sc32, seed_of(100), *g32.outputs(), s32)
    torch.cuda.synchronize()
    g32.p.set_profiling(True)
    g32.p.reset_profiling()
    res = [g32.outputs() for _ in range(3)]
    busy(s32)
    for i in range(3):
        g32.seed_call(sc32, seed_of(i), res[i][0], res[i][1], s32)
    torch.cuda.synchronize()
    got = (g32.launches("prologue_ahead"), g32.launches("prologue"))
    g32.p.set_profiling(False)
    assert got == (0, 3), got
    for i in range(3):
        w = g32.alone(v32, seed_of(i))
        assert np.array_equal(u64(res[i][0]), w[0]) and np.array_equal(u64(res[i][1]), w[1]), f"l=32 call {i}"
    o1, o2 = g32.oracle(v32, seed_of(1))
    assert np.array_equal(u64(res[1][0]), o1) and np.array_equal(u64(res[1][1]), o2), "l=32 oracle"


def mixed():
    """seed, _rs, seed, explicit back to back on a busy stream, twice over: every result as in order"""
    for geometry in ("A", "C"):
        n, k, l, moduli, _ = GEOMETRIES[geometry]
        g = Setup(n, k, l, moduli)
        s = torch.cuda.Stream(device=DEV)
        vals = [scalars_of(n, 20 + i) for i in range(8)]
        scs = [dev_u64(v) for v in vals]
        outs = [g.outputs() for _ in range(8)]
        rnds = {i: g.explicit(seed_of(20 + i)) for i in (3, 7)}
        g.seed_call(scs[0], seed_of(100), *g.outputs(), s)
        torch.cuda.synchronize()
        c0 = (1 << 32) - 1
        with P.DeviceRandomness(g.p, S, c0) as st:
            g.p.set_profiling(True)
            g.p.reset_profiling()
            busy(s)
            for i in range(8):
                if i % 4 in (0, 2):
                    g.seed_call(scs[i], seed_of(20 + i), outs[i][0], outs[i][1], s)
                elif i % 4 == 1:
                    g.rs_call(scs[i], st, outs[i][0], outs[i][1], s)
                else:
                    g.explicit_call(scs[i], rnds[i][0], outs[i][0], outs[i][1], s)
            torch.cuda.synchronize()
            got = (g.launches("prologue_ahead"), g.launches("prologue"))
            g.p.set_profiling(False)
            assert 1 <= got[0] <= 3 and sum(got) == 8, got     # the seed calls but the first
            assert st.counter(s) == c0 + 2
        for i in range(8):
            seed = P.DeviceRandomness.call_seed(S, c0 + i // 4) if i % 4 == 1 else seed_of(20 + i)
            w1, w2 = g.alone(vals[i], seed)
            assert np.array_equal(u64(outs[i][0]), w1) and np.array_equal(u64(outs[i][1]), w2), f"geometry {geometry} call {i}"


def concurrent():
    """two threads, two streams, one context, six calls each on busy streams"""
    n, k, l, moduli, _ = GEOMETRIES["A"]
    g = Setup(n, k, l, moduli)
    streams = [torch.cuda.Stream(device=DEV) for _ in range(2)]
    vals = [[scalars_of(n, 200 + 10 * t + i) for i in range(6)] for t in range(2)]
    scs = [[dev_u64(v) for v in vals[t]] for t in range(2)]
    outs = [[g.outputs() for _ in range(6)] for _ in range(2)]
    g.seed_call(scs[0][0], seed_of(100), *g.outputs(), streams[0])
    torch.cuda.synchronize()
    g.p.set_profiling(True)
    g.p.reset_profiling()
    errors = []
    gate = threading.Barrier(2)

    def run(t):
        try:
            torch.cuda.set_device(0)
            busy(streams[t])
            gate.wait(timeout=30)
            for i in range(6):
                g.seed_call(scs[t][i], seed_of(200 + 10 * t + i), outs[t][i][0], outs[t][i][1], streams[t])
        except BaseException as e:   # noqa: BLE001  (reported by the main thread)
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=60)
    assert not any(th.is_alive() for th in threads) and not errors, errors
    torch.cuda.synchronize()
    got = (g.launches("prologue_ahead"), g.launches("prologue"))
    g.p.set_profiling(False)
    assert got[0] >= 2 and sum(got) == 12, got
    for t in range(2):
        for i in range(6):
            w1, w2 = g.alone(vals[t][i], seed_of(200 + 10 * t + i))
            assert np.array_equal(u64(outs[t][i][0]), w1) and np.array_equal(u64(outs[t][i][1]), w2), f"thread {t} call {i}"


CASES = {f.__name__: f for f in (exact, ordered, paths, mixed, concurrent)}

if __name__ == "__main__":
    assert torch.cuda.is_available()
    CASES[sys.argv[1]](*sys.argv[2:])
    print("AHEAD_OK")
