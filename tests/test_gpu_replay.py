"""GPU suite: every device entry that opens with a clear, run FIVE times in one workspace and one set of buffers, bit for bit against
numpy (tests/_replay.py).  The families change from run to run -- two values, eight, n, one, eight again -- so a later run meets the
state a different earlier run left.  Two modes tell stale workspace state from graph replay: `eager` is five plain calls, `graph` is a
warm-up, one capture and four replays.  Outputs are pre-filled with a sentinel before every run, the payloads of the in-place sorts
start every run above a base of their own, and every message carries the run, its family and the raw fault words of the workspace."""
import ctypes

import numpy as np
import pytest

import _replay as rp
import _unique as un

pytestmark = pytest.mark.gpu

RUNS = len(rp.RUNS)


def _torch_dtype(w):
    import torch

    return torch.int32 if w == 32 else torch.int64


def _signed(w):
    return np.int32 if w == 32 else np.int64


def _zeros(n, w=32):
    import torch

    return torch.zeros(n, dtype=_torch_dtype(w), device="cuda")


def _put(t, words):
    import torch

    t.copy_(torch.from_numpy(np.ascontiguousarray(words).view(_signed(8 * words.dtype.itemsize)).copy()))


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


def _stream():
    import torch

    return int(torch.cuda.current_stream().cuda_stream)


def _words(ws, *offsets):
    """The raw 32-bit words of the workspace at the byte offsets, read through torch: which device check fired."""
    return ["0x%08X" % (int(ws[o:o + 4].view(_torch_dtype(32)).item()) & 0xFFFFFFFF) for o in offsets]


class Unit:
    """One entry's buffers, its call, and what a run must leave.  load(run) | call() | verify(run, tell)."""
    ws = None
    fault_offsets = (0,)

    def __init__(self, gpu, cell):
        self.gpu, self.L, self.cell, self.n = gpu, gpu.lib(), cell, cell["n"]

    def faults(self):
        return _words(self.ws, *self.fault_offsets) if self.ws is not None else []


def _say(tell, *more):
    """One string (pytest cuts a long tuple short): the cell, the mode, the run, its family, the fault words, and what differs."""
    return " | ".join(str(part) for part in tuple(tell) + more)


def _same(got, want, tell, what):
    assert np.array_equal(got, want), _say(tell, what, "first mismatch at", int(np.flatnonzero(got != want)[0]))


# ---- the 32-bit sorts: lsdsort_keys_device, lsdsort_u32_device, lsdsort_pairs_u32_device, lsdsort_multi_u32_device ------------------
class Sort32(Unit):
    def __init__(self, gpu, cell):
        import torch

        super().__init__(gpu, cell)
        entry = cell["entry"]
        self.key_type = cell.get("key_type", "uint32")
        self.descending = cell.get("descending", False)
        self.payloads = {"lsdsort_u32_device": 0, "lsdsort_pairs_u32_device": 1}.get(entry, cell.get("payloads", 0))
        n = self.n
        self.dk = _zeros(n)
        self.dv = [_zeros(n) for _ in range(self.payloads)]
        need = self.L.lsdsort_workspace_bytes(n, 8, self.payloads)
        self.ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        self.ptrs = (ctypes.c_void_p * max(self.payloads, 1))(*[v.data_ptr() for v in self.dv])
        dk, dv, ws, L = self.dk, self.dv, self.ws, self.L
        code = un.KEY_CODE[self.key_type]
        self.call = {
            "lsdsort_keys_device": lambda: L.lsdsort_keys_device(dk.data_ptr(), dv[0].data_ptr() if dv else None, ws.data_ptr(), need, n, 8, code,
                                                                 int(self.descending), _stream()),
            "lsdsort_u32_device": lambda: L.lsdsort_u32_device(dk.data_ptr(), ws.data_ptr(), need, n, 8, _stream()),
            "lsdsort_pairs_u32_device": lambda: L.lsdsort_pairs_u32_device(dk.data_ptr(), dv[0].data_ptr(), ws.data_ptr(), need, n, 8, _stream()),
            "lsdsort_multi_u32_device": lambda: L.lsdsort_multi_u32_device(dk.data_ptr(), self.ptrs, self.payloads, ws.data_ptr(), need, n, 8, _stream()),
        }[entry]

    def load(self, run):
        _put(self.dk, rp.keys(self.n, self.key_type, run))
        for k, v in enumerate(self.dv):
            _put(v, rp.payload(self.n, run, k))

    def verify(self, run, tell):
        status = self.L.lsdsort_check_device(self.ws.data_ptr(), None)
        assert status == 0, _say(tell, "lsdsort_check_device", status)
        bits = rp.keys(self.n, self.key_type, run)
        want, want_pay = rp.oracle_sort(bits, self.key_type, self.descending, [rp.payload(self.n, run, k) for k in range(self.payloads)])
        _same(_host(self.dk, np.uint32), want, tell, "keys")
        for k, v in enumerate(self.dv):
            _same(_host(v, np.uint32), want_pay[k], tell, "payload %d" % k)


# ---- 64-bit keys: lsdsort_keys64_device -------------------------------------------------------------------------------------------
class Sort64(Unit):
    def __init__(self, gpu, cell):
        import torch

        super().__init__(gpu, cell)
        n, self.val_bits = self.n, cell["val_bits"]
        self.dk = _zeros(n, 64)
        self.dv = _zeros(n) if self.val_bits else None
        need = self.L.lsdsort_wide_workspace_bytes(n, 8, 64, self.val_bits)
        self.ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        # the sticky word, and the fault word of the sorts inside: the arrays of low and high key words lie between them
        self.fault_offsets = (0, rp.ALIGN + 2 * (-(-4 * n // rp.ALIGN) * rp.ALIGN))
        dk, dv, ws, L, code = self.dk, self.dv, self.ws, self.L, un.KEY_CODE[cell["key_type"]]
        self.call = lambda: L.lsdsort_keys64_device(dk.data_ptr(), dv.data_ptr() if dv is not None else None, self.val_bits, ws.data_ptr(), need,
                                                    n, 8, code, int(cell["descending"]), _stream())

    def load(self, run):
        _put(self.dk, rp.keys(self.n, self.cell["key_type"], run))
        if self.dv is not None:
            _put(self.dv, rp.payload(self.n, run))

    def verify(self, run, tell):
        status = self.L.lsdsort_wide_check_device(self.ws.data_ptr(), self.n, 8, 64, self.val_bits, None)
        assert status == 0, _say(tell, "lsdsort_wide_check_device", status)
        bits = rp.keys(self.n, self.cell["key_type"], run)
        want, want_pay = rp.oracle_sort(bits, self.cell["key_type"], self.cell["descending"], [rp.payload(self.n, run)])
        _same(_host(self.dk, np.uint64), want, tell, "keys")
        if self.dv is not None:
            _same(_host(self.dv, np.uint32), want_pay[0], tell, "payload")


# ---- lsdsort_unique_device ----------------------------------------------------------------------------------------------------------
class Unique(Unit):
    def __init__(self, gpu, cell):
        import torch

        super().__init__(gpu, cell)
        n, self.key_type, outputs = self.n, cell["key_type"], cell["outputs"]
        self.w = w = un.width_of(self.key_type)
        self.dk, self.out = _zeros(n, w), _zeros(n, w)
        self.arrays = {name: _zeros(n) for name in outputs}
        self.num = _zeros(1)
        self.positions = positions = int("first" in outputs or "inverse" in outputs)
        code = un.KEY_CODE[self.key_type]
        need = self.L.lsdsort_unique_workspace_bytes(n, code, positions)
        self.ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        self.code = code
        self.fault_offsets = (0, rp.unique_sort_offset(n, w, positions))   # the unit's own word, and the first of the sort's workspace inside
        ptr = {name: (self.arrays[name].data_ptr() if name in self.arrays else None) for name in ("counts", "first", "inverse")}
        dk, out, num, ws, L = self.dk, self.out, self.num, self.ws, self.L
        self.call = lambda: L.lsdsort_unique_device(dk.data_ptr(), n, code, int(cell["descending"]), out.data_ptr(), ptr["counts"], ptr["first"],
                                                    ptr["inverse"], num.data_ptr(), ws.data_ptr(), need, _stream())

    def load(self, run):
        _put(self.dk, rp.keys(self.n, self.key_type, run))
        self.out.fill_(rp.SENT[self.w])
        for t in list(self.arrays.values()) + [self.num]:
            t.fill_(rp.SENT[32])

    def verify(self, run, tell):
        status = self.L.lsdsort_unique_check_device(self.ws.data_ptr(), self.n, self.code, self.positions, None)
        assert status == 0, _say(tell, "lsdsort_unique_check_device", status)
        bits = rp.keys(self.n, self.key_type, run)
        want = un.oracle_unique(bits, self.key_type, self.cell["descending"])
        m = want["keys"].size
        assert int(_host(self.num, np.uint32)[0]) == m, _say(tell, "count", int(_host(self.num, np.uint32)[0]), m)
        got = _host(self.out, bits.dtype)
        _same(got[:m], want["keys"], tell, "keys")
        assert (got[m:] == bits.dtype.type(rp.SENT[self.w])).all(), _say(tell, "keys written past the count",)
        for name in ("counts", "first"):
            if name in self.arrays:
                got = _host(self.arrays[name], np.uint32)
                _same(got[:m], want[name], tell, name)
                assert (got[m:] == rp.SENT[32]).all(), _say(tell, name, "written past the count")
        if "inverse" in self.arrays:
            _same(_host(self.arrays["inverse"], np.uint32), want["inverse"], tell, "inverse")
        _same(_host(self.dk, bits.dtype), bits, tell, "the input")


# ---- lsdsort_digit_histograms_u32_device: the clear of a caller's table ----------------------------------------------------------------
class Histograms(Unit):
    def __init__(self, gpu, cell):
        super().__init__(gpu, cell)
        n, r = self.n, cell["radix_bits"]
        self.dk = _zeros(n)
        self.hist = _zeros((32 // r) << r)
        dk, hist, L = self.dk, self.hist, self.L
        self.call = lambda: L.lsdsort_digit_histograms_u32_device(dk.data_ptr(), n, r, hist.data_ptr(), _stream())

    def load(self, run):
        _put(self.dk, rp.keys(self.n, "uint32", run))
        self.hist.fill_(rp.SENT[32])

    def verify(self, run, tell):
        want = rp.oracle_histograms(rp.keys(self.n, "uint32", run), self.cell["radix_bits"])
        _same(_host(self.hist, np.uint32), want.reshape(-1), tell, "table")


# ---- lsdsort_msb_partition_u32_device, lsdsort_splitter_partition_u32_device -------------------------------------------------------------
class Partition(Unit):
    def __init__(self, gpu, cell):
        import torch

        super().__init__(gpu, cell)
        n = self.n
        self.by_value = cell["entry"] == "lsdsort_splitter_partition_u32_device"
        self.bits = bits = cell["log2_buckets"] if self.by_value else cell["msb_bits"]
        self.dk, self.out = _zeros(n), _zeros(n)
        self.counts = _zeros(1 << bits, 64)
        need = self.L.lsdsort_msb_partition_workspace_bytes(n, bits)
        self.ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        self.values = rp.splitters(n, bits) if self.by_value else ()
        self.host_values = (ctypes.c_uint32 * max(len(self.values), 1))(*self.values)
        dk, out, counts, ws, L = self.dk, self.out, self.counts, self.ws, self.L
        if self.by_value:
            self.call = lambda: L.lsdsort_splitter_partition_u32_device(dk.data_ptr(), out.data_ptr(), n, bits, self.host_values if bits else None,
                                                                        counts.data_ptr(), ws.data_ptr(), need, _stream())
        else:
            self.call = lambda: L.lsdsort_msb_partition_u32_device(dk.data_ptr(), out.data_ptr(), n, bits, counts.data_ptr(), ws.data_ptr(), need,
                                                                   _stream())

    def load(self, run):
        _put(self.dk, rp.keys(self.n, "uint32", run))
        self.out.fill_(rp.SENT[32])
        self.counts.fill_(rp.SENT[64])

    def verify(self, run, tell):
        status = self.L.lsdsort_check_device(self.ws.data_ptr(), None)
        assert status == 0, _say(tell, "lsdsort_check_device", status)
        bits = rp.keys(self.n, "uint32", run)
        bucket = rp.splitter_buckets(bits, self.values) if self.by_value else rp.msb_buckets(bits, self.bits)
        want, want_counts = rp.oracle_partition(bits, bucket, 1 << self.bits)
        _same(_host(self.counts, np.uint64), want_counts, tell, "counts")
        _same(_host(self.out, np.uint32), want, tell, "keys by bucket")
        _same(_host(self.dk, np.uint32), bits, tell, "the input")


UNITS = {
    "lsdsort_keys_device": Sort32,
    "lsdsort_u32_device": Sort32,
    "lsdsort_pairs_u32_device": Sort32,
    "lsdsort_multi_u32_device": Sort32,
    "lsdsort_keys64_device": Sort64,
    "lsdsort_unique_device": Unique,
    "lsdsort_digit_histograms_u32_device": Histograms,
    "lsdsort_msb_partition_u32_device": Partition,
    "lsdsort_splitter_partition_u32_device": Partition,
}


def _five_runs(gpu, cell, mode):
    import torch

    assert gpu.lib().lsdsort_prepare_device() == 0
    unit = UNITS[cell["entry"]](gpu, cell)

    def step(run, launch):
        unit.load(run)
        status = launch()
        assert status in (None, 0), (rp.cell_id(cell), mode, "run", run, "status", status)
        torch.cuda.synchronize()
        unit.verify(run, (rp.cell_id(cell), mode, "run", run, rp.RUNS[run][0], "fault words", unit.faults()))

    if mode == "eager":
        for run in range(RUNS):
            step(run, unit.call)
        return
    step(0, unit.call)   # the warm-up: device set-up stays out of the capture
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        status = unit.call()
    assert status == 0, (rp.cell_id(cell), "capture", status)
    for run in range(1, RUNS):
        step(run, graph.replay)


@pytest.mark.parametrize("mode", rp.MODES)
@pytest.mark.parametrize("cell", rp.CELLS, ids=rp.cell_id)
def test_five_runs_in_one_workspace(gpu, cell, mode):
    if cell.get("small", True):
        _five_runs(gpu, cell, mode)
        return
    gpu.set_small_sort(False)   # the chained form at a size the one-launch sort would take
    try:
        _five_runs(gpu, cell, mode)
    finally:
        gpu.set_small_sort(True)
