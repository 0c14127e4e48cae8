"""Keys on the device and words back from it, for the GPU suites of the row entries (a helper module: no fixtures, no pytest
settings).  The guard zones are _guarded.py's and _guarded16.py's; the oracle is _key_oracle.py's."""
import numpy as np
import torch

DTYPES = {"uint16": torch.int16, "int16": torch.int16, "float16": torch.float16, "bfloat16": torch.bfloat16,
          "uint32": torch.int32, "int32": torch.int32, "float32": torch.float32}
_WORD = {2: (torch.int16, np.int16, np.uint16), 4: (torch.int32, np.int32, np.uint32)}


def to_dev(keys, key_type, offset=0):
    """the keys ([rows, cols] uint16 or uint32 bits, by key_type) on the device as a contiguous [rows, cols] view `offset` elements
    into a 512-byte aligned buffer"""
    rows, cols = keys.shape
    size = 2 if key_type.endswith("16") else 4
    word, host_word, _ = _WORD[size]
    flat = torch.empty(rows * cols + offset, dtype=word, device="cuda")
    assert flat.data_ptr() % 512 == 0
    view = flat[offset:].view(rows, cols)
    view.copy_(torch.from_numpy(np.ascontiguousarray(keys).view(host_word)))
    assert view.is_contiguous() and view.data_ptr() % 16 == (size * offset) % 16
    return view.view(DTYPES[key_type])


def bits(t):
    """uint16 bit patterns of a 16-bit tensor, uint32 of a 32-bit one, on the host"""
    word, _, host_bits = _WORD[t.element_size()]
    return t.contiguous().view(word).cpu().numpy().view(host_bits)


def stream_ptr(stream=None):
    return int((stream or torch.cuda.current_stream()).cuda_stream)


def fault_word(ws):
    return int(ws[:4].view(torch.int32).item()) & 0xFFFFFFFF


def assert_equal(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, f"{what}: shape {a.shape} against {b.shape}"
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        at = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} words differ, first at {at}: got {a[at]:#x} want {b[at]:#x}")


def captured(call):
    """a graph of one `call`, captured after a warm-up on a side stream"""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()   # warm-up: device set-up stays out of the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    return g
