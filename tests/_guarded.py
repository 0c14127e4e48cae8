"""Guard zones for the device entries of include/lsdsort.h (a helper module: no fixtures, no pytest settings).

Every device entry takes raw pointers and a byte count and promises to stay inside them.  torch's caching allocator rounds
every request up (512 B, or 2 MiB blocks), so a store a few bytes past an array, or past the workspace figure the library
reports, lands in slack and no result check sees it.  Here every array passed to an entry is a view into a larger buffer
whose two outer zones hold a sentinel: GUARD elements (GUARD bytes for a workspace) on either side, twice the largest tile.
The view can be put at any 16-byte phase, which selects the 16-byte or the key-by-key load path of the kernels that choose
between them by the base address.

    whole, view = guarded(host_array, skip_bytes)      view.data_ptr() % 16 == skip_bytes
    whole, ws = guarded_workspace(nbytes)              exactly nbytes, 256-byte aligned; pass nbytes as workspace_bytes
    assert_intact(keys=whole, workspace=wwhole)        both zones of every buffer still hold the sentinel
    assert_unchanged(view, host_array)                 for inputs the header calls read-only

The sentinel is 0x7E7E7E7E (0x7E7E7E7E7E7E7E7E for 64-bit elements, 0x7E for bytes): neither the padding value 0xFFFFFFFF
nor, by construction (without_sentinel), a value of the test inputs.
"""
import numpy as np
import torch

GUARD = 1 << 16                     # elements on either side of an array, bytes on either side of a workspace
SENT32 = 0x7E7E7E7E
SENT64 = 0x7E7E7E7E7E7E7E7E
SENT8 = 0x7E

_DEVICE_DTYPE = {4: torch.int32, 8: torch.int64}
_SENTINEL = {torch.int32: SENT32, torch.int64: SENT64, torch.uint8: SENT8}


def without_sentinel(host_array):
    """The array with every element that equals the sentinel of its width changed in its lowest bit (in place)."""
    sent = {4: SENT32, 8: SENT64}[host_array.dtype.itemsize]
    bits = host_array.view({4: np.uint32, 8: np.uint64}[host_array.dtype.itemsize])
    bits[bits == sent] ^= bits.dtype.type(1)
    return host_array


def guarded(host_array, skip_bytes=0):
    """(whole, view): `whole` is a device tensor of GUARD + n + GUARD elements filled with the sentinel, `view` its n payload
    elements holding `host_array` (32- or 64-bit elements, taken bit for bit), with view.data_ptr() % 16 == skip_bytes."""
    host = np.ascontiguousarray(host_array)
    size = host.dtype.itemsize
    assert size in (4, 8) and 0 <= skip_bytes < 16 and skip_bytes % size == 0, (host.dtype, skip_bytes)
    dtype = _DEVICE_DTYPE[size]
    n = host.size
    lead = skip_bytes // size
    raw = torch.full((GUARD + n + GUARD + 16 // size,), _SENTINEL[dtype], dtype=dtype, device="cuda")
    assert raw.data_ptr() % 512 == 0, "torch buffers are 512-byte aligned: every skip gives the alignment it names"
    whole = raw[lead:lead + GUARD + n + GUARD]
    view = whole[GUARD:GUARD + n]
    if n:
        view.copy_(torch.from_numpy(np.array(host.reshape(-1).view({4: np.int32, 8: np.int64}[size]))))   # a writable copy
    assert (whole.data_ptr() + GUARD * size) % 16 == skip_bytes and (n == 0 or view.data_ptr() == whole.data_ptr() + GUARD * size)
    return whole, view


def guarded_workspace(nbytes):
    """(whole, view): a uint8 buffer with GUARD bytes of 0x7E on either side of a 256-byte-aligned view of exactly `nbytes`
    bytes -- the library's figure as reported, not rounded; the entry is passed `nbytes` as its workspace_bytes."""
    nbytes = int(nbytes)
    whole = torch.full((GUARD + nbytes + GUARD,), SENT8, dtype=torch.uint8, device="cuda")
    view = whole[GUARD:GUARD + nbytes]
    assert whole.data_ptr() % 512 == 0 and (whole.data_ptr() + GUARD) % 256 == 0
    return whole, view


def ptr(view):
    """The address to pass for a view: NULL for an empty one."""
    return view.data_ptr() if view is not None and view.numel() else None


def assert_intact(*wholes, **named):
    """Both zones of every buffer still hold the sentinel (compared on the device); the message names the buffer, the side
    and the first changed offset (in elements: counted back from the view's first element, or on from its end)."""
    items = [(f"buffer {i}", w) for i, w in enumerate(wholes)] + list(named.items())
    for name, whole in items:
        if whole is None:
            continue
        sent = _SENTINEL[whole.dtype]
        n = whole.numel() - 2 * GUARD
        for side, zone in (("before", whole[:GUARD]), ("after", whole[GUARD + n:])):
            if bool((zone == sent).all()):
                continue
            bad = (zone != sent).nonzero().reshape(-1)
            first = int(bad[0]) if side == "after" else int(bad[-1])
            where = f"{first} elements past its end" if side == "after" else f"{GUARD - first} elements before its start"
            value = int(zone[first]) & ((1 << (8 * whole.element_size())) - 1)
            raise AssertionError(f"guard zone {side} {name} was written: {bad.numel()} elements changed, the nearest one "
                                 f"{where} (zone offset {first}) now holds {value:#x}")


def assert_unchanged(view, host_array, what="a read-only input"):
    host = np.ascontiguousarray(host_array).reshape(-1)
    bits = {4: np.uint32, 8: np.uint64}[host.dtype.itemsize]
    got = view.cpu().numpy().view(bits)
    want = host.view(bits)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{what} was changed: {bad.size} elements, first at {bad[0]}: {got[bad[0]]:#x} was {want[bad[0]]:#x}")
