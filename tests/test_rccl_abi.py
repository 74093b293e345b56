"""The mix bus over RCCL behind the C ABI (include/fwgpu.h "the mix bus over RCCL"; the node being computed:
nodes/sum.rs:111-133).  CPU tier: the host harness library (real host code, fake HIP runtime, a launch stub that computes the node)
against tests/host_harness/fakerccl.cpp — N ranks as threads of one process, each with its own context and communicator: the dlopen
path, the unique-id hand-over, the in-place all-reduce, and the VALUES of the all-gather route (16-byte flag slots at r * n_sil, the
in-place send, callers without flags) over a sequence of calls that grows, shrinks and regrows the bus on one communicator — in a
child process whose fresh device memory is poisoned, because the flags of a caller that passes none come from a buffer nobody writes
per call.  GPU tier: the same sequence through the REAL k_bus_sum_ordered at world 2, 3, 5 and 8 (ranks as threads on the one device,
tests/host_harness/devrccl.cpp doing the gathers: the real librccl refuses two ranks on one device), and the REAL librccl at world 1;
N > 1 over real RCCL on hardware stays unmeasured."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import fwapi

ROOT = fwapi.ROOT
ID_BYTES = 128


def fake_rccl():
    d = os.path.join(ROOT, "tests", "host_harness")
    so, src = os.path.join(d, "_fakerccl.so"), os.path.join(d, "fakerccl.cpp")
    if not os.path.exists(so) or os.path.getmtime(src) > os.path.getmtime(so):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-Wall", "-o", so, src, "-lpthread"])
    return so


def dev_rccl():
    """tests/host_harness/devrccl.cpp: the entry points for ranks that are threads on ONE real device (needs only the ROCm headers:
    it finds the HIP runtime the process has already loaded)"""
    d = os.path.join(ROOT, "tests", "host_harness")
    so, src = os.path.join(d, "_devrccl.so"), os.path.join(d, "devrccl.cpp")
    if not os.path.exists(so) or os.path.getmtime(src) > os.path.getmtime(so):
        rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                               "-o", so, src, "-ldl", "-lpthread"])
    return so


# ---------------------------------------------------------------------------------------------- the sequence of calls
# One communicator, stereo, 32-frame blocks: (blocks, who passes flags, floats short of a whole last block).  Call 1 sizes every
# buffer; calls 2 and 3 pass no flags and have more blocks — whether a buffer must grow for them depends on the world size (see
# growth_model); call 4 mixes ranks with and without flags; call 5 shrinks, with a ragged last block; call 6 is call 3's size again.
FRAMES = 32
SEQUENCE = [(3, "all", 0), (8, "none", 0), (16, "none", 0), (16, "all but rank 0", 0), (5, "all", 4), (16, "none", 0)]


def sequence_call(world, k):
    """(parts, flags as passed per rank (None: that rank passes no flags), expected out, expected flags) of call k"""
    from test_bus_exchange import random_buses, topsum_model

    blocks, who, ragged = SEQUENCE[k]
    parts, sils = random_buses(np.random.default_rng(1000 * world + k), world, blocks, FRAMES, ragged=ragged)
    passed = [s if who == "all" or (who == "all but rank 0" and r > 0) else None for r, s in enumerate(sils)]
    want, want_sil = topsum_model(parts, passed, FRAMES)
    return parts, passed, want, want_sil


def devbuf_cap(cap, need):
    """DevBuf::ensure (fwgpu_ctx.h): the capacity after a request of `need` bytes — at least 256 bytes; a first allocation gets an
    eighth, at least 4096 bytes, of headroom; a regrow a quarter"""
    if cap and need <= cap:
        return cap
    want = max(need, 256)
    if not cap:
        return want + max(want // 8, 4096) if want <= (16 << 20) else want
    return want + want // 4


def growth_model(world):
    """per call of SEQUENCE: which of a rank's (gathered, gathered_sil, zero_sil) buffers are too small for it"""
    caps, grows = [0, 0, 0], []
    for blocks, _, ragged in SEQUENCE:
        n_floats = blocks * FRAMES * 2 - ragged
        n_sil = (blocks * 2 + 15) & ~15
        need = (world * n_floats * 4, world * n_sil, n_sil)
        grows.append([need[i] > caps[i] for i in range(3)])
        caps = [devbuf_cap(caps[i], need[i]) for i in range(3)]
    return grows


def test_the_sequence_has_a_call_that_sends_more_flag_bytes_without_any_buffer_growing():
    # at world 1 call 1 leaves 768 + 4096 bytes of bus and 256 + 4096 bytes in both flag buffers; call 3 (4096 bytes of bus,
    # 32 flag bytes where 16 were cleared) fits all three — no allocation, so nothing that only runs when a buffer grows runs
    assert growth_model(1) == [[True] * 3] + [[False] * 3] * 5
    assert SEQUENCE[2][0] * 2 > 16 >= SEQUENCE[0][0] * 2
    # ... while larger worlds outgrow the gathered bus again and again (both kinds of call are in the sequence)
    assert all(growth_model(w)[2][0] for w in (2, 3, 5, 8, 17))


def _first_difference(world, k, r, out, osil, want, want_sil):
    a, b = out.view(np.uint32), want.view(np.uint32)
    if not np.array_equal(a, b):
        i = int(np.flatnonzero(a != b)[0])
        return "world %d, call %d %r, rank %d: %d floats differ, first at %d (block %d): got %r, want %r" % (
            world, k + 1, SEQUENCE[k], r, int((a != b).sum()), i, i // (FRAMES * 2), out[i], want[i])
    if not np.array_equal(osil.reshape(want_sil.shape), want_sil):
        return "world %d, call %d %r, rank %d: silence flags %r, want %r" % (world, k + 1, SEQUENCE[k], r, osil.tolist(), want_sil.reshape(-1).tolist())
    return None


def _join(ts, limit):
    for t in ts:
        t.join(limit)
    return [i for i, t in enumerate(ts) if t.is_alive()]


def _host_sequence(world):
    """(child process, FWGPU_POISON=1, FWGPU_RCCL_LIB = the fake) the sequence on the host harness, ranks as threads"""
    L = fwapi.hostonly_lib()
    uid = (C.c_uint8 * ID_BYTES)()
    assert L.fwgpu_rccl_unique_id(uid) == 0, L.fwgpu_rccl_last_error()
    cases = [sequence_call(world, k) for k in range(len(SEQUENCE))]
    grows = growth_model(world)
    got, errs, allocs = [[None] * len(SEQUENCE) for _ in range(world)], [], []

    def rank(r):
        try:
            cx = make_ctx(L)
            m = L.fwgpu_rccl_comm_create(cx, uid, world, r)
            assert m, L.fwgpu_last_error(cx)
            for k, (parts, passed, want, want_sil) in enumerate(cases):
                n = parts[r].size
                out = np.full(n, np.nan, dtype=np.float32)
                osil = np.full(want_sil.size, 9, dtype=np.uint8)
                flags = None if passed[r] is None else np.ascontiguousarray(passed[r].reshape(-1))
                before = L.fwh_alloc_count()
                rc = L.fwgpu_bus_allgather_ordered(m, parts[r].ctypes.data_as(C.c_void_p), None if flags is None else flags.ctypes.data_as(C.c_void_p),
                                                   out.ctypes.data_as(C.c_void_p), osil.ctypes.data_as(C.c_void_p), n, FRAMES, 2)
                assert rc == 0, (k, L.fwgpu_last_error(cx))
                allocs.append(L.fwh_alloc_count() - before)
                got[r][k] = (out, osil)
            assert L.fwgpu_rccl_comm_destroy(m) == 0
            L.fwgpu_ctx_destroy(cx)
        except BaseException as ex:  # noqa: BLE001
            errs.append((r, repr(ex)))

    ts = [threading.Thread(target=rank, args=(r,), daemon=True) for r in range(world)]
    for t in ts:
        t.start()
    stuck = _join(ts, 60)
    if stuck or errs:
        print("ranks failed:", errs, "still running:", stuck)
        return 1
    if world == 1:  # (one thread: the harness's allocation counter is exact) a rank allocates exactly when the model says a buffer is short
        if allocs != [sum(g) for g in grows] or allocs[2] != 0:
            print("allocations per call %r, DevBuf model %r" % (allocs, grows))
            return 1
    if L.fwh_violation() not in (b"", None):
        print("host harness violation:", L.fwh_violation())
        return 1
    for k, (parts, passed, want, want_sil) in enumerate(cases):  # call by call: the first call that differs is the one reported
        for r in range(world):
            d = _first_difference(world, k, r, got[r][k][0], got[r][k][1], want, want_sil)
            if d:
                print("MISMATCH", d)
                return 1
    print("sequence ok: world %d" % world)
    return 0


def _device_sequence(worlds, calls):
    """(child process, FWGPU_POISON=1) the sequence on the device: every rank a thread with its own context and stream.  Every tensor
    is made and read on the main thread; after any failure nothing more is started on the device (os._exit)."""
    import torch  # (first: libfwgpu binds to the HIP runtime torch has mapped — tests/conftest.py)

    import firewheel_amd as fa

    def bail(*what):
        print(*what, flush=True)
        os._exit(1)

    L = fa.load_library()
    for world in worlds:
        cases = {k: sequence_call(world, k) for k in calls}
        dev = {}
        for k, (parts, passed, want, want_sil) in cases.items():
            for r in range(world):
                dev[r, k] = (torch.from_numpy(parts[r]).cuda(),
                             None if passed[r] is None else torch.from_numpy(np.ascontiguousarray(passed[r].reshape(-1))).cuda(),
                             torch.full((parts[r].size,), float("nan"), dtype=torch.float32, device="cuda"),
                             torch.full((want_sil.size,), 9, dtype=torch.uint8, device="cuda"))
        torch.cuda.synchronize()
        ctxs = [fa.FirewheelGpuCtx(48000, 256, 0, 2) for _ in range(world)]
        uid = (C.c_uint8 * ID_BYTES)()
        if L.fwgpu_rccl_unique_id(uid) != 0:
            bail("unique id:", L.fwgpu_rccl_last_error())
        errs = []

        def rank(r):
            try:
                cx = ctxs[r]
                m = L.fwgpu_rccl_comm_create(cx.c, uid, world, r)
                assert m, L.fwgpu_last_error(cx.c)
                for k in calls:
                    bus, flags, out, osil = dev[r, k]
                    rc = L.fwgpu_bus_allgather_ordered(m, C.c_void_p(bus.data_ptr()), None if flags is None else C.c_void_p(flags.data_ptr()),
                                                       C.c_void_p(out.data_ptr()), C.c_void_p(osil.data_ptr()), bus.numel(), FRAMES, 2)
                    assert rc == 0, (k, L.fwgpu_last_error(cx.c))
                cx.synchronize()
                assert L.fwgpu_rccl_comm_destroy(m) == 0, L.fwgpu_last_error(cx.c)
            except BaseException as ex:  # noqa: BLE001
                errs.append((r, repr(ex)))

        ts = [threading.Thread(target=rank, args=(r,), daemon=True) for r in range(world)]
        for t in ts:
            t.start()
        stuck = _join(ts, 60)
        if stuck or errs:
            bail("world %d: ranks failed:" % world, errs, "still running:", stuck)
        torch.cuda.synchronize()
        for k in calls:
            for r in range(world):
                d = _first_difference(world, k, r, dev[r, k][2].cpu().numpy(), dev[r, k][3].cpu().numpy(), cases[k][2], cases[k][3])
                if d:
                    bail("MISMATCH", d)
        for cx in ctxs:
            cx.close()
        print("sequence ok: world %d" % world, flush=True)


def _child(mode, *args, **env):
    e = dict(os.environ, FWGPU_POISON="1", **env)
    if "FWGPU_RCCL_LIB" not in env:
        e.pop("FWGPU_RCCL_LIB", None)
    return subprocess.run([sys.executable, os.path.abspath(__file__), mode] + [str(a) for a in args], env=e, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("world", [1, 2, 3, 5, 8, 17])
def test_allgather_values_over_growing_and_shrinking_calls_in_poisoned_memory_on_the_host_harness(world):
    """every rank's output and flags after each of the six calls equal the model's, in a process whose fresh "device" memory is 0xCB:
    rank r's slot at r * n_sil, the in-place send, and the zeros a caller without flags sends — whichever way its buffers got their
    size"""
    r = _child("host", world, FWGPU_RCCL_LIB=fake_rccl())
    assert r.returncode == 0 and "sequence ok: world %d" % world in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def make_ctx(L):
    c = L.fwgpu_ctx_create(0, 48000, 64, 0, 2, None)
    assert c
    return c


@pytest.mark.parametrize("world", [1, 2, 5, 8])
def test_allreduce_and_allgather_through_the_abi_on_the_host_harness(world):
    os.environ["FWGPU_RCCL_LIB"] = fake_rccl()  # (read when the harness library first loads an RCCL: once per process)
    L = fwapi.hostonly_lib()
    uid = (C.c_uint8 * ID_BYTES)()
    assert L.fwgpu_rccl_unique_id(uid) == 0, L.fwgpu_rccl_last_error()
    n = 4 * 64 * 2  # 4 blocks x 64 frames x 2 channels
    rng = np.random.default_rng(5)
    parts = [rng.standard_normal(n).astype(np.float32) for _ in range(world)]
    sil = [np.zeros(4 * 2, dtype=np.uint8) for _ in range(world)]
    sil[world - 1][3] = 1
    expect = parts[0].copy()
    for r in range(1, world):
        expect = expect + parts[r]  # rank order, one f32 rounding per add: the fake ring's order
    got, errs = [None] * world, []
    gathered = [[] for _ in range(world)]
    from test_bus_exchange import topsum_model

    want, want_sil = topsum_model(parts, [x.reshape(4, 2) for x in sil], 64)

    def rank(r):
        try:
            cx = make_ctx(L)
            m = L.fwgpu_rccl_comm_create(cx, uid, world, r)
            assert m, L.fwgpu_last_error(cx)
            w, k = C.c_uint32(), C.c_uint32()
            assert L.fwgpu_rccl_comm_info(m, C.byref(w), C.byref(k)) == 0 and (w.value, k.value) == (world, r)
            bus = parts[r].copy()
            assert L.fwgpu_bus_allreduce_rccl(m, bus.ctypes.data_as(C.c_void_p), n) == 0, L.fwgpu_last_error(cx)
            got[r] = bus
            out = np.full(n, np.nan, dtype=np.float32)
            osil = np.full(8, 9, dtype=np.uint8)
            for i in range(2):  # (second call: the scratch is reused)
                out[:], osil[:] = np.nan, 9
                rc = L.fwgpu_bus_allgather_ordered(m, parts[r].ctypes.data_as(C.c_void_p), sil[r].ctypes.data_as(C.c_void_p),
                                                   out.ctypes.data_as(C.c_void_p), osil.ctypes.data_as(C.c_void_p), n, 64, 2)
                assert rc == 0, L.fwgpu_last_error(cx)
                gathered[r].append((out.copy(), osil.copy()))
            assert L.fwgpu_bus_allgather_ordered(m, parts[r].ctypes.data_as(C.c_void_p), None, out.ctypes.data_as(C.c_void_p), None, n + 2, 64, 2) < 0
            assert L.fwgpu_rccl_comm_destroy(m) == 0
            L.fwgpu_ctx_destroy(cx)
        except BaseException as ex:  # noqa: BLE001
            errs.append((r, repr(ex)))

    ts = [threading.Thread(target=rank, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(60)
    assert not errs, errs
    assert L.fwh_violation() in (b"", None), L.fwh_violation()
    for r in range(world):
        assert np.array_equal(got[r].view(np.uint32), expect.view(np.uint32)), r
        assert len(gathered[r]) == 2
        for i, (out, osil) in enumerate(gathered[r]):  # all-gather + ordered sum: the model's bits and flags on every rank, both calls
            assert np.array_equal(out.view(np.uint32), want.view(np.uint32)), (r, i)
            assert np.array_equal(osil.reshape(4, 2), want_sil), (r, i)


def test_bad_arguments_are_refused_without_a_collective():
    os.environ["FWGPU_RCCL_LIB"] = fake_rccl()
    L = fwapi.hostonly_lib()
    cx = make_ctx(L)
    uid = (C.c_uint8 * ID_BYTES)()
    assert L.fwgpu_rccl_unique_id(uid) == 0
    assert not L.fwgpu_rccl_comm_create(cx, uid, 0, 0)
    assert not L.fwgpu_rccl_comm_create(cx, uid, 2, 2)
    assert not L.fwgpu_rccl_comm_create(cx, None, 1, 0)
    assert L.fwgpu_rccl_unique_id(None) < 0
    assert L.fwgpu_bus_allreduce_rccl(None, None, 4) < 0
    assert L.fwgpu_rccl_comm_destroy(None) == 0
    L.fwgpu_ctx_destroy(cx)


@pytest.mark.gpu
def test_real_rccl_at_world_one_on_the_device():
    import torch

    import firewheel_amd as fa

    L = fa.load_library()
    cx = fa.FirewheelGpuCtx(48000, 256, 0, 2)
    uid = (C.c_uint8 * ID_BYTES)()
    assert L.fwgpu_rccl_unique_id(uid) == 0, L.fwgpu_rccl_last_error()
    m = L.fwgpu_rccl_comm_create(cx.c, uid, 1, 0)
    assert m, L.fwgpu_last_error(cx.c)
    n = 8 * 256 * 2
    bus = torch.randn(n, device="cuda", dtype=torch.float32)
    bus.view(8, 256, 2)[2, :, 1] = 0.0  # block 2, channel 1 is silent: cleared AND flagged, as fwgpu_process_blocks_device_flags leaves it
    ref = bus.clone()
    sil = torch.zeros(8 * 2, dtype=torch.uint8, device="cuda")
    sil[5] = 1  # a one-port sum copies the port and passes its flag on (sum.rs:58-65)
    torch.cuda.synchronize()
    assert L.fwgpu_bus_allreduce_rccl(m, C.c_void_p(bus.data_ptr()), n) == 0, L.fwgpu_last_error(cx.c)
    out = torch.full((n,), float("nan"), device="cuda")
    osil = torch.full((16,), 7, dtype=torch.uint8, device="cuda")
    assert L.fwgpu_bus_allgather_ordered(m, C.c_void_p(ref.data_ptr()), C.c_void_p(sil.data_ptr()), C.c_void_p(out.data_ptr()),
                                         C.c_void_p(osil.data_ptr()), n, 256, 2) == 0, L.fwgpu_last_error(cx.c)
    cx.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(bus.view(torch.int32), ref.view(torch.int32))
    assert torch.equal(out.view(torch.int32), ref.view(torch.int32))
    assert osil.cpu().tolist() == sil.cpu().tolist()
    assert L.fwgpu_rccl_comm_destroy(m) == 0
    cx.close()


@pytest.mark.gpu
def test_allgather_values_at_world_2_3_5_8_through_the_real_kernel_on_one_device():
    """the six calls at world 2, 3, 5 and 8 on device tensors: ranks are threads with a context and a stream each, the gathers are
    device-to-device copies into the real slot layout (tests/host_harness/devrccl.cpp), the sum is the real k_bus_sum_ordered —
    unmasked (2, 3) and masked (5, 8) — in poisoned device memory"""
    r = _child("device", 2, 3, 5, 8, FWGPU_RCCL_LIB=dev_rccl())
    assert r.returncode == 0 and "sequence ok: world 8" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


@pytest.mark.gpu
def test_real_rccl_at_world_one_without_flags_over_growing_calls_in_poisoned_memory():
    """the real librccl, one rank (as test_real_rccl_at_world_one_on_the_device), calls 1, 2, 3 and 6 of the sequence: a caller
    without flags whose later calls fit the buffers the first one sized"""
    r = _child("real")
    assert r.returncode == 0 and "sequence ok: world 1" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


if __name__ == "__main__":  # (the poisoned runs: a fresh child process each — FWGPU_POISON and FWGPU_RCCL_LIB are read once per process)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if sys.argv[1] == "host":
        sys.exit(_host_sequence(int(sys.argv[2])))
    if sys.argv[1] == "device":
        _device_sequence([int(a) for a in sys.argv[2:]], list(range(len(SEQUENCE))))
    elif sys.argv[1] == "real":
        _device_sequence([1], [0, 1, 2, 5])
    else:
        sys.exit(2)
