"""Guard zones for 16-bit key arrays (a helper module: no fixtures, no pytest settings) -- the 2-byte counterpart of _guarded.py,
whose `guarded` handles 4- and 8-byte elements only.  The workspace and the 32-bit payloads keep using _guarded.py.

    whole, view = guarded16(bits, skip_bytes, dtype)   view.data_ptr() % 16 == skip_bytes, any even skip 0..14
    assert_intact16(keys=whole)                        both zones still hold the sentinel

`whole` is an int16 tensor of GUARD + n + GUARD elements filled with 0x7E7E; `view` its n payload elements holding `bits` (uint16
bit patterns) seen as `dtype` (torch.int16, float16 or bfloat16).  The zones are compared, never the payload, so the inputs may
hold the sentinel's value."""
import numpy as np
import torch

GUARD = 1 << 16      # elements on either side
SENT16 = 0x7E7E


def guarded16(bits, skip_bytes=0, dtype=torch.int16):
    host = np.ascontiguousarray(bits, dtype=np.uint16).reshape(-1)
    assert 0 <= skip_bytes < 16 and skip_bytes % 2 == 0, skip_bytes
    n = host.size
    lead = skip_bytes // 2
    raw = torch.full((GUARD + n + GUARD + 8,), SENT16, dtype=torch.int16, device="cuda")
    assert raw.data_ptr() % 512 == 0, "torch buffers are 512-byte aligned: every skip gives the alignment it names"
    whole = raw[lead:lead + GUARD + n + GUARD]
    view = whole[GUARD:GUARD + n]
    if n:
        view.copy_(torch.from_numpy(host.view(np.int16).copy()))
    assert (whole.data_ptr() + 2 * GUARD) % 16 == skip_bytes
    return whole, view.view(dtype)


def bits_of(view):
    """The uint16 bit patterns of a 16-bit tensor, on the host."""
    return view.view(torch.int16).cpu().numpy().view(np.uint16)


def assert_intact16(*wholes, **named):
    items = [(f"buffer {i}", w) for i, w in enumerate(wholes)] + list(named.items())
    for name, whole in items:
        n = whole.numel() - 2 * GUARD
        for side, zone in (("before", whole[:GUARD]), ("after", whole[GUARD + n:])):
            if bool((zone == SENT16).all()):
                continue
            bad = (zone != SENT16).nonzero().reshape(-1)
            first = int(bad[0]) if side == "after" else int(bad[-1])
            where = f"{first} elements past its end" if side == "after" else f"{GUARD - first} elements before its start"
            raise AssertionError(f"guard zone {side} {name} was written: {bad.numel()} elements changed, the nearest one {where} "
                                 f"now holds {int(zone[first]) & 0xFFFF:#x}")
