"""Driver of tests/test_handle_buffers.py: the entry points that keep buffers with the handle, called in a fixed sequence against a library whose HIP calls are
tests/host_sim/fake_hip.cpp's (device memory is host memory, kernels do nothing).  After every call it records the status and the nine numbers of fakehip_image:
[hash of the live device allocations, their count, their bytes, kernel launches, H2D copies, H2D bytes, D2D copies, memsets, pinned bytes ever allocated].

    python tests/handle_buffers_driver.py <library> [trace|growth|all]

prints one JSON line.  `trace`: three sessions, create -> open -> update (pods + nodes with flags) -> update (pods only) -> best_nodes x2 -> ops_apply x2 -> reset ->
reopen -> close -> destroy; two builds of the library that make the same HIP calls print the same line.  `growth`: a warm handle, then a call large enough to regrow
each buffer, then the same call again."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import kai_testlib as T  # noqa: E402

pkg = T.pkg; abi = pkg.abi; syn = pkg.synth
lib = C.CDLL(sys.argv[1])
Q, A, Op, Res = abi.KaiNodeQuery, abi.KaiNodeAnswer, abi.KaiOp, abi.KaiApplyResult
lib.kai_best_nodes.argtypes = [C.c_void_p, C.POINTER(Q), C.c_int32, C.POINTER(C.c_uint32), C.c_int32, C.POINTER(A)]
lib.kai_ops_apply.argtypes = [C.c_void_p, C.POINTER(Op), C.c_int64, C.c_uint32, C.POINTER(Res)]
PENDING, RUNNING = abi.POD_STATUS["Pending"], abi.POD_STATUS["Running"]


def image():
    img = (C.c_uint64 * 9)(); lib.fakehip_image(img); return [int(x) for x in img]


def sessions():
    yield "C2 at 30 %", syn.config(1, 0.3)[:2], True
    yield "C5 at 20 %", syn.config(4, 0.2)[:2], True
    s, c, _ = syn.config(1, 0.2); syn.add_fractions(s, 7, frac=0.3)
    yield "C2 at 20 % with fractions", (s, c), False  # (kai_ops_apply refuses a session with shared-GPU requests)


class Handle:
    def __init__(self, snap, cfg):
        self.snap, self.h = snap, C.c_void_p()
        self.P, self.N = snap.n_pods, snap.n_nodes
        self.pending = np.nonzero(snap.arrays["pod_status"] == PENDING)[0].astype(np.int64)
        self.rc_create = lib.kai_core_create(C.byref(cfg), 1, None, C.byref(self.h))

    def open(self):
        st = self.snap.as_struct(); return lib.kai_session_open(self.h, C.byref(st))

    def update(self, n_pods, nodes=False):
        """The first n_pods pending pods run on nodes 0, 1, ...; with `nodes`, nodes 0 and 3 get new flags as well."""
        pods = self.pending[:n_pods]
        assert len(pods) == n_pods
        kw = dict(nodes=[0, 3], node_flags=[0x1, 0x0]) if nodes else {}
        d, keep = pkg.core.delta_struct(pods, [RUNNING] * n_pods, np.arange(n_pods) % self.N, **kw)
        return lib.kai_session_update(self.h, C.byref(d))

    def best_nodes(self, m):
        """m queries: the pods cycled, the node sets -1 / 0 / 1 (two sets of all nodes)."""
        qs = np.zeros(m, np.dtype([("pod", "<i4"), ("nodeset", "<i4"), ("flags", "<u4"), ("pad", "<u4")]))
        qs["pod"] = np.arange(m) % self.P; qs["nodeset"] = np.arange(m) % 3 - 1
        assert qs.itemsize == C.sizeof(Q)
        W = (self.N + 31) // 32
        words = (C.c_uint32 * (2 * W))(*([0xffffffff] * (2 * W)))
        out = (A * m)()
        return lib.kai_best_nodes(self.h, qs.ctypes.data_as(C.POINTER(Q)), m, words, 2, out)

    def ops_apply(self, n, flags=0):
        """n ALLOCATE operations, one statement each, on distinct pending pods."""
        pods = self.pending[:n]
        assert len(pods) == n
        arr = (Op * n)(*[Op(i, 0, int(p), i % self.N, 0, i, 0) for i, p in enumerate(pods)])
        r = Res()
        return lib.kai_ops_apply(self.h, arr, n, flags, C.byref(r))

    def destroy(self):
        return lib.kai_core_destroy(self.h)


def trace():
    out = {}
    for name, (snap, cfg), with_ops in sessions():
        rows = []
        def step(call, rc):
            rows.append([call, int(rc), image()])
        h = Handle(snap, cfg)
        step("create", h.rc_create)
        step("open", h.open())
        step("update pods + nodes", h.update(5, nodes=True))
        step("update pods", h.update(5))
        step("best_nodes", h.best_nodes(7)); step("best_nodes again", h.best_nodes(7))
        if with_ops:
            step("ops_apply", h.ops_apply(4)); step("ops_apply again", h.ops_apply(4))
        step("reset", lib.kai_session_reset(h.h))
        step("reopen", h.open())
        step("close", lib.kai_session_close(h.h))
        step("destroy", h.destroy())
        out[name] = rows
    return out


def growth():
    """Per entry point and session: the image before, after a cold and a warm small call, after the large call and after the large call again."""
    out = {}
    c2, c5 = syn.config(1, 0.3)[:2], syn.config(4, 0.2)[:2]
    n_pending_c2 = int((c2[0].arrays["pod_status"] == PENDING).sum())
    cases = [("best_nodes", c2, lambda h, n: h.best_nodes(n), 3, 8192),
             ("ops_apply", c5, lambda h, n: h.ops_apply(n), 2, 8192),
             ("update", c5, lambda h, n: h.update(n), 3, 4096),
             # the sizes of tests/test_gpu_handle_buffers.py (C2 at 30 %): every one regrows its buffer
             ("ops_apply check-only, C2", c2, lambda h, n: h.ops_apply(n, flags=abi.APPLY_CHECK_ONLY), 2, n_pending_c2),
             ("update, C2", c2, lambda h, n: h.update(n), 3, min(c2[0].n_pods // 2, n_pending_c2))]
    for name, (snap, cfg), call, small, large in cases:
        h = Handle(snap, cfg)
        rcs = [h.rc_create, h.open()]
        imgs = [image()]
        for n in (small, small, large, large):
            rcs.append(call(h, n)); imgs.append(image())
        rcs.append(h.destroy())
        out[name] = dict(rcs=rcs, images=imgs, after_destroy=image(), small=small, large=large)
    return out


if __name__ == "__main__":
    mode = sys.argv[2] if len(sys.argv) > 2 else "trace"
    res = trace() if mode == "trace" else growth() if mode == "growth" else dict(trace=trace(), growth=growth())
    print(json.dumps(res))
