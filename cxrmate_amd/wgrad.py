"""The scheduler of the training step's second stream. Weight-gradient work (split-K TN GEMMs, depthwise-conv tap sums, parameter-gradient row
sums) only feeds the optimiser, never the dX chain: inside an overlap() context it is issued on a side stream so that these atomics-/latency-bound
kernels overlap the MFMA-bound dX GEMMs and attention kernels of the main stream."""
from __future__ import annotations

import contextlib
import ctypes as _ct
import os
import warnings

import torch

from ._lib import LIB, STRUCTS

_DEV_INDEX = None
_RAW_OVERRIDE = None    # raw handle of the weight-gradient stream while flush() issues collected launches


def raw_stream():
    """Raw hipStream_t of torch's current stream (fast path: no Stream object, no device queries -- this runs ~1500x per step)."""
    global _DEV_INDEX
    if _RAW_OVERRIDE is not None:
        return _RAW_OVERRIDE
    if _DEV_INDEX is None:
        _DEV_INDEX = torch.cuda.current_device()
    return torch._C._cuda_getCurrentRawStream(_DEV_INDEX)


TnPending = STRUCTS["cxr_tn_pending"]     # a weight gradient whose sum over the token splits is still to be added to C / dbias

_TN_WS_FLOATS = 16 << 20    # scratch of the immediate path: 16 M floats (64 MB) cover every shape of this model
_TN_CHUNK = 64 << 20        # floats per arena buffer of the deferred path (256 MB)


class Scheduler:
    """All state of the weight-gradient stream; `scheduler` below is the one instance. What keeps it correct:
    (a) Launches collected by defer() are issued (flush) before any reduce and before any synchronisation with the side stream.
    (b) A destination with a pending split sum is settled (reduce) before anything else accumulates into it: the batched reduce is a plain
        read-modify-write, so two entries naming one C (tied parameters, a weight used twice), or a one-split launch into a pending C, would race.
    (c) The arena cursor is rewound only by reduce(): the same stream orders the next GEMM's partial tiles behind that reduce launch.
    (d) Operands of collected launches are kept alive until join(), not pinned with record_stream; nothing may overwrite one in place before that
        join -- the side stream runs arbitrarily far behind the main stream.
    (e) The persistent NT GEMM kernels are off from begin() to join(), while weight-gradient kernels may run beside the main stream.
    (f) On an exception overlap() calls discard(): every collected launch, kept operand and pending sum is dropped and the arena rewound, so
        nothing of a failed step is launched later by an unrelated one.
    settle() = flush + reduce is due wherever something may READ a weight gradient: the joins, the fork points of the gradient all-reduce and of the
    early optimiser update, other side-stream work that consumes a GEMM's result, the end of an overlap() context."""

    def __init__(self):
        env = os.environ.get
        self.side = None            # the active side stream (None: everything on torch's current stream)
        self.owned = None           # the stream overlap() switches to, created on first use
        self.deferred = []          # launches waiting for the next fork point (closures issuing C-ABI launches on the side stream)
        self.kept = []              # their operands, kept alive until the next join()
        self.batch = max(1, int(env("CXR_WGRAD_BATCH", "4")))      # launches per fork event
        # Deferred split sums (CXR_TN_DEFER=0: every GEMM followed by its own reduce launch). Each deferred GEMM gets scratch of its own from a bump
        # allocator over a few large buffers (288 GB of HBM: the ~2 GB of partial tiles a step leaves behind are not a constraint); reduce() adds
        # all pending sums with one launch per 40 and hands the scratch back.
        self.tn_defer = env("CXR_TN_DEFER", "1") != "0"
        self.tn_defer_floats = int(env("CXR_TN_DEFER_MB", "64")) << 18      # pending partial tiles that trigger a reduce launch (MB -> floats)
        self.tn_arena = {}          # device index -> [buffers, index of the current one, floats used in it]
        self.tn_pending = []        # (TnPending, tensors kept alive)
        self.tn_ptrs = set()        # destinations of the pending sums
        # Immediate path: (device index, raw stream handle) -> fp32 scratch of the deterministic split-K GEMM (launches of one stream are serial). An
        # output beyond it (splits * I_pad * J_pad floats, more than 192 splits) falls back to fp32 atomics inside cxr_gemm_tn_bf16 -- reported
        # once per shape, never silent
        self.tn_ws = {}
        self.tn_fallback_seen = set()
        self.exclusive_on = True
        self.excl_always = env("CXR_GEMM_EXCL_ALWAYS") == "1"      # lab switch: persistent GEMM kernels also beside the weight-gradient stream
        self.skip = env("CXR_WGRAD_SKIP") == "1"                   # TIMING EXPERIMENT ONLY (wrong gradients): no weight-gradient GEMM is launched
        if self.skip:
            if env("CXR_DEBUG_TIMING") != "1":
                raise RuntimeError("CXR_WGRAD_SKIP=1 drops every Linear weight gradient (a timing experiment): it is only honoured together with "
                                   "CXR_DEBUG_TIMING=1")
            warnings.warn("CXR_WGRAD_SKIP=1: NO Linear weight gradient is computed in this process -- timing experiment, training results are wrong",
                          RuntimeWarning, stacklevel=1)

    # ------------------------------------------------------------------------------------------------ streams
    def stream(self):
        return self.side

    def owned_stream(self):
        """The stream overlap() runs on, for a join() issued after its context has ended (deferred joins)."""
        return self.owned

    def issuing(self):
        """The side stream while flush() is issuing collected launches on it (the stream raw_stream() then names), else None."""
        return self.side if _RAW_OVERRIDE is not None else None

    @contextlib.contextmanager
    def overlap(self):
        """Context: run weight-gradient kernels on the side stream."""
        if self.owned is None and os.environ.get("CXR_WGRAD_OVERLAP", "1") != "0":      # 0: A/B switch, everything on one stream
            # CXR_WGRAD_PRIORITY: stream priority of the weight-gradient stream (default: torch's default = lowest; negative = higher)
            self.owned = torch.cuda.Stream(priority=int(os.environ.get("CXR_WGRAD_PRIORITY", "0")))
        self.flush()
        prev, self.side = self.side, self.owned
        try:
            try:
                yield
            except BaseException:
                self.discard()                              # the step failed: nothing of it is launched later by an unrelated step
                raise
            self.settle()                                   # launches still collected for this stream are issued on it, their split sums added
        finally:
            self.side = prev

    def on_stream(self, *tensors):
        """Context: torch's current stream is the side stream, behind everything issued on either stream so far; `tensors` are pinned to it."""
        return _OnStream(tensors)

    # ------------------------------------------------------------------------------------------------ collected launches
    def defer(self, fn, *tensors):
        """Issue `fn` (C-ABI launches only, nothing allocated) on the weight-gradient stream. Ordering against the main stream costs an event
        record on the MAIN stream -- a barrier packet that keeps the next main-stream kernel from starting under the tail of the previous one:
        ~9 us each, 145 of them = 1.3 ms of a 41-ms step when every weight-gradient launch had its own. The launches are therefore collected and
        issued in batches of CXR_WGRAD_BATCH behind ONE event (flush)."""
        if self.side is None:
            fn()
            return
        self.deferred.append(fn)
        self.kept.append(tensors)
        if len(self.deferred) >= self.batch:
            self.flush()

    def flush(self):
        """Issue the collected weight-gradient launches: one event on the main stream (their operands are complete), the side stream waits for it."""
        global _RAW_OVERRIDE
        if not self.deferred:
            return
        side = self.side
        assert side is not None, "deferred weight-gradient launches outlived their stream (overlap() exits through flush)"
        ev = torch.cuda.Event()
        ev.record()
        side.wait_event(ev)
        _RAW_OVERRIDE = side.cuda_stream
        try:
            for fn in self.deferred:
                fn()
        finally:
            _RAW_OVERRIDE = None
            self.deferred.clear()

    def reduce(self, side=None):
        """Add every pending split sum to its gradient (one launch per 40 sums, on the side stream, behind the GEMMs that left the partial tiles)."""
        if not self.tn_pending:
            return
        side = self.side if side is None else side
        assert side is not None, "pending weight-gradient sums outlived their stream"
        arr = (TnPending * len(self.tn_pending))(*[d for d, _ in self.tn_pending])
        LIB.call("cxr_gemm_tn_reduce_batch", _ct.addressof(arr), len(self.tn_pending), side.cuda_stream)
        self._tn_forget()

    def _tn_forget(self):
        self.tn_pending.clear()
        self.tn_ptrs.clear()
        for ar in self.tn_arena.values():
            ar[1] = ar[2] = 0

    def settle(self):
        self.flush()
        self.reduce()

    def discard(self):
        """Drop collected launches and pending sums without issuing them (error path of overlap(); the exclusive flag stays as it is)."""
        self.deferred.clear()
        self.kept.clear()
        self._tn_forget()

    def join(self, stream=None):
        """stream: the weight-gradient stream to join when called outside the overlap() context that launched on it (deferred joins)"""
        self.flush()
        stream = self.side if stream is None else stream
        self.reduce(stream)
        if stream is not None:
            torch.cuda.current_stream().wait_stream(stream)
        self.kept.clear()
        self.exclusive(True)                                # nothing runs beside the main stream any more

    def exclusive(self, on: bool):
        """on: NT GEMM launches may use the persistent one-workgroup-per-CU kernels (csrc/gemm_ws.hip, gemm_pk.hip: 144 KB of LDS each). The
        backward passes turn it off while weight-gradient kernels run beside the main stream (begin) -- such a workgroup cannot share a CU with
        them and the kernels' static work partition would wait for the last CU to free up (measured: 43.9 -> 45.8 ms per step)."""
        if bool(on) != self.exclusive_on:
            self.exclusive_on = bool(on)
            LIB.call("cxr_gemm_set_exclusive", int(bool(on)))

    def begin(self):
        """Start of a backward pass: from here on weight-gradient kernels may be running on the side stream (until join)."""
        if self.side is not None and not self.excl_always:
            self.exclusive(False)

    def mark(self):
        """Event at the side stream's current position (None without a side stream): lets a later consumer wait for exactly the work issued so
        far (the W^T transposes of a forward pass) instead of joining the whole weight-gradient backlog."""
        if self.side is None:
            return None
        self.settle()
        ev = torch.cuda.Event()
        ev.record(self.side)
        return ev

    def wait(self, ev):
        if ev is not None:
            torch.cuda.current_stream().wait_event(ev)

    # ------------------------------------------------------------------------------------------------ split-K scratch and pending sums (ops.gemm_tn)
    def tn_settle_dest(self, out, dbias):
        """Invariant (b), in front of a GEMM that adds into out / dbias (stream order then serialises the two, as before the deferral)."""
        if self.tn_ptrs and (out.data_ptr() in self.tn_ptrs or (dbias is not None and dbias.data_ptr() in self.tn_ptrs)):
            self.reduce()

    def tn_deferring(self):
        return self.tn_defer and self.issuing() is not None

    def tn_scratch(self, device, n):
        """`n` floats for the partial tiles of one deferred GEMM."""
        ar = self.tn_arena.get(device.index)
        if ar is None:
            ar = self.tn_arena[device.index] = [[], 0, 0]
        bufs = ar[0]
        n = (n + 63) // 64 * 64
        while True:
            if ar[1] < len(bufs) and ar[2] + n <= bufs[ar[1]].numel():
                out = bufs[ar[1]][ar[2]: ar[2] + n]
                ar[2] += n
                return out
            if ar[1] < len(bufs):
                ar[1] += 1
                ar[2] = 0
                continue
            bufs.append(torch.empty(max(n, _TN_CHUNK), dtype=torch.float32, device=device))

    def tn_add_pending(self, pend, out, dbias):
        if pend.splits <= 1:
            return
        self.tn_pending.append((pend, (out, dbias)))
        self.tn_ptrs.add(out.data_ptr())
        if dbias is not None:
            self.tn_ptrs.add(dbias.data_ptr())
        # ... but not for long: the partial tiles should still be in the 256-MB Infinity Cache when the reduce reads them (with every sum of a
        # step pending, ~2 GB of partial tiles went out to HBM and came back: the step got 0.16 ms SLOWER than with one reduce launch per GEMM)
        ar = self.tn_arena[out.device.index]
        if len(self.tn_pending) >= 40 or ar[1] > 0 or ar[2] >= self.tn_defer_floats:
            self.reduce()

    def tn_scratch_immediate(self, stream, device, R, I, J):
        """The per-stream scratch of a GEMM that reduces at once; warns when the shape cannot use the deterministic partial-tile path (the launch
        plan comes from the library: cxr_gemm_tn_plan)."""
        key = (device.index, stream)
        ws = self.tn_ws.get(key)
        if ws is None:
            ws = self.tn_ws[key] = torch.empty(_TN_WS_FLOATS, dtype=torch.float32, device=device)
        if (I, J) not in self.tn_fallback_seen and I * J > (1 << 20):
            splits, need = _ct.c_int(0), _ct.c_long(0)
            LIB.call("cxr_gemm_tn_plan", int(R), int(I), int(J), _ct.byref(splits), _ct.byref(need))
            if splits.value > 1 and (need.value > _TN_WS_FLOATS or splits.value > 192):
                self.tn_fallback_seen.add((I, J))
                warnings.warn(f"weight-gradient GEMM {I}x{J} over {R} rows: {splits.value} splits need {need.value} scratch floats (> {_TN_WS_FLOATS}) "
                              "-> fp32 atomics, the sum order (last bits of the gradient) is not reproducible for this shape")
        return ws


class _OnStream:
    def __init__(self, tensors):
        self.tensors = tensors

    def __enter__(self):
        self.side = scheduler.side
        if self.side is not None:
            scheduler.settle()                              # collected launches come first on the side stream; what follows may read a weight gradient
            self.side.wait_stream(torch.cuda.current_stream())
            self.ctx = torch.cuda.stream(self.side)
            self.ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if self.side is not None:
            self.ctx.__exit__(*exc)
            for t in self.tensors:
                if t is not None:
                    t.record_stream(self.side)
        return False


scheduler = Scheduler()
stream, owned_stream, overlap, on_stream = scheduler.stream, scheduler.owned_stream, scheduler.overlap, scheduler.on_stream
defer, flush, reduce, settle, discard, join = scheduler.defer, scheduler.flush, scheduler.reduce, scheduler.settle, scheduler.discard, scheduler.join
exclusive, begin, mark, wait = scheduler.exclusive, scheduler.begin, scheduler.mark, scheduler.wait
