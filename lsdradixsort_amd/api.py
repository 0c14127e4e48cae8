"""The Python face of ``liblsdsort.so`` over the C-ABI (include/lsdsort.h).

PyTorch is plumbing only: device memory and the current HIP stream.  All computation happens in the library; nothing here
falls back to PyTorch or the CPU.  The sort path keeps the reference's names (``LSDRadixSort/LSDRadixSort.cu``):
``GPULSDRadixSort`` (.cu:839), ``BuildHistograms`` (.cu:660), ``LSDRadixSortKernel`` -> ``RankScatter`` (.cu:795).

A map of the file, in its order:

- host-pointer entries (``sort``, ``sort_pairs``);
- the shared plumbing: ``_dev`` (the tensor check), ``_key_type``, ``_stream`` / ``_on_stream``, ``_workspace`` (the one
  workspace path, over ``_temp_workspace``), ``_check_fault``, ``_ptr``; then the library's switches;
- the 32-bit sorts: plain, multi, typed, segmented (``sort_rows``);
- the 32-bit row selects (``_keys32``, ``_select_code32``, ``_select_outputs``, ``_ranks``): top-k, k-th value, multi-rank,
  and ``_Rows``, the flatten / restore helper of every torch-shaped ``*_rows`` wrapper; quantiles;
- the wide sorts (``sort64``) and the 16-bit sort (``sort16``), which share ``_sort_1d``;
- the 16-bit rows (``_keys16``, ``_logits16``, ``_per_row``, ``_row_out``, ``_fill16``): selects, per-row ranks, the two
  filters, the draw, the log-probabilities, the row sort;
- the run units (``_word_keys``, ``_run_outputs``, ``_run_result``, ``_slice_by_count``): run-length, unique, the two reduces;
- the timed sort, the stage entries and the partitions.

Every device wrapper has the same five steps, in this order:

1. check the arguments (nothing below is reached with a bad one, the library least of all);
2. allocate the outputs under ``_on_stream(stream)``;
3. take the workspace from ``_workspace``;
4. call the entry, through ``check``;
5. ``_check_fault`` where ``check_fault`` is set and kernels ran at all.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import errors
from ._lib import LsdsortTiming, lib
from .errors import KEY_TYPES_16, KEY_TYPES_32, KEY_TYPES_64, LSDSORT_ALGO_ONESWEEP, LSDSORT_ALGO_STAGED, check  # noqa: F401

# exactly what __init__.py re-exports from here (tests/test_python_face_cpu.py)
__all__ = [
    "sort", "sort_pairs", "to_device", "to_host", "workspace_bytes", "alloc_workspace", "workspace_form", "workspace_half", "tile_keys",
    "set_tile_config", "set_xcd_chunk", "set_hybrid", "set_half_hop", "set_small_sort", "set_pass_skipping", "set_rank_method", "rank_method",
    "GPULSDRadixSort", "GPULSDRadixSortTimed", "GPUSortMulti", "GPUSortTyped", "GPUSortWide", "sort64",
    "GPUSort16", "keys16_workspace_bytes", "set_keys16_route", "sort16", "GPUTopK16", "topk16_workspace_bytes", "topk16_rows",
    "GPUSortRows16", "rows16_workspace_bytes", "set_rows16_route", "sort_rows16",
    "GPUSortSegmented", "segmented_workspace_bytes", "sort_rows", "GPUTopK", "topk_workspace_bytes", "topk_rows",
    "GPUKth", "kth_workspace_bytes", "kthvalue_rows", "median_rows",
    "GPUKthMulti", "kth_multi_workspace_bytes", "quantile_rows", "quantile_ranks",
    "GPUKth16", "kth16_workspace_bytes", "kthvalue16_rows", "median16_rows",
    "GPUKth16Multi", "kth16_multi_workspace_bytes", "quantile16_rows",
    "GPUKth16PerRow", "kth16_perrow_workspace_bytes", "GPUTopK16Filter", "topk16_filter_workspace_bytes", "topk16_filter_rows",
    "GPUTopP16Filter", "topp16_filter_workspace_bytes", "topp16_filter_rows",
    "GPUSample16", "sample16_workspace_bytes", "sample16_rows",
    "GPULogprob16", "logprob16_workspace_bytes", "logprobs16_rows", "top_logprobs16_rows",
    "GPURunLength", "GPUUnique", "rle_workspace_bytes", "unique_workspace_bytes", "unique", "unique_consecutive",
    "GPUReduceRuns", "GPUReduceByKey", "reduce_runs_workspace_bytes", "reduce_by_key_workspace_bytes", "reduce_by_key", "reduce_consecutive",
    "BuildHistograms", "BuildOffsets", "RankScatter", "DigitHistograms",
    "MSBPartition", "SplitterPartition", "ThresholdPartition", "sharded_thresholds",
]


def _torch():
    import torch

    return torch


# ------------------------------------------------------------------------------ host-pointer entries
def _host_u32(a: np.ndarray, name: str) -> np.ndarray:
    if not isinstance(a, np.ndarray) or a.dtype != np.uint32 or a.ndim != 1 or not a.flags.c_contiguous:
        raise TypeError(f"{name} must be a contiguous 1-D numpy.uint32 array")
    if not a.flags.writeable:
        raise TypeError(f"{name} must be writeable (sorted in place)")
    return a


def sort(keys: np.ndarray, radix_bits: int = 8) -> np.ndarray:
    """``sort(uint32_t* keys, size_t n)``: host array, in place, ascending (``lsdsort_u32_ex``)."""
    _host_u32(keys, "keys")
    check(lib().lsdsort_u32_ex(keys.ctypes.data, keys.size, radix_bits, 1), "lsdsort_u32_ex")
    return keys


def sort_pairs(keys: np.ndarray, vals: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """Key/value sort, stable by key, host arrays in place (``lsdsort_pairs_u32``)."""
    _host_u32(keys, "keys")
    _host_u32(vals, "vals")
    if keys.size != vals.size:
        raise ValueError("keys and vals differ in length")
    check(lib().lsdsort_pairs_u32(keys.ctypes.data, vals.ctypes.data, keys.size), "lsdsort_pairs_u32")
    return keys, vals


# ------------------------------------------------------------------------------ device plumbing
def to_device(a: np.ndarray, device: str = "cuda"):
    """uint32 host array -> int32 device tensor with the same bits."""
    torch = _torch()
    a = np.ascontiguousarray(a, dtype=np.uint32)
    return torch.from_numpy(a.view(np.int32)).to(device)


def to_host(t) -> np.ndarray:
    """int32 device tensor -> uint32 host array with the same bits."""
    return t.detach().cpu().numpy().view(np.uint32)


def _dtype_name(dtype) -> str:
    """``torch.bfloat16`` -> "bfloat16": what the messages call a dtype, and the key-type name of a tensor sorted as what it is."""
    return str(dtype).replace("torch.", "")


def _dev(t, name: str, dtypes=None, dims=None, contiguous: bool = True):
    """The tensor check of every wrapper: ``t`` is a CUDA tensor of one of ``dtypes`` (default: int32, holding uint32 bit
    patterns), with one of ``dims`` dimensions where that is given, and contiguous -- except where the wrapper sorts a copy it
    makes itself."""
    torch = _torch()
    dtypes = dtypes or (torch.int32,)
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype in dtypes and (t.is_contiguous() or not contiguous)
            and (dims is None or t.dim() in dims)):
        shape = "" if dims is None else " or ".join(f"{d}-D" for d in dims) + " "
        kinds = " or ".join(_dtype_name(d) for d in dtypes)
        raise TypeError(f"{name}: a {'contiguous ' if contiguous else ''}{shape}{kinds} CUDA tensor")
    return t


def _payload(d_vals, n: int, name: str = "d_vals", dtypes=None, what: str = "vals"):
    """A payload array: the tensor check, and as long as the keys."""
    _dev(d_vals, name, dtypes)
    if d_vals.numel() != n:
        raise ValueError(f"keys and {what} differ in length")
    return d_vals


def _key_type(key_type: str, table: dict) -> int:
    """The header's code of a key type name; ``table`` is KEY_TYPES_32, KEY_TYPES_64 or KEY_TYPES_16."""
    if key_type not in table:
        raise ValueError("key_type: " + " or ".join(f'"{name}"' for name in table) + f", got {key_type!r}")
    return table[key_type]


def _stream(stream=None) -> int:
    torch = _torch()
    s = stream if stream is not None else torch.cuda.current_stream()
    return int(s.cuda_stream)


def _on_stream(stream):
    """Context in which torch allocates and enqueues on ``stream``; ``None``: on the current stream, as it does anyway."""
    torch = _torch()
    return torch.cuda.stream(stream)


def _temp_workspace(nbytes: int, device, stream):
    """The one place a workspace tensor is made; ``_workspace`` and ``alloc_workspace`` are its only callers.  A wrapper returns
    while its kernels are still running, so a temporary workspace must belong to THEIR stream: allocated under ``stream`` (where
    that is not torch's current stream, ``None``), the caching allocator orders the block's reuse after the sort's kernels instead
    of after whatever the current stream is doing."""
    torch = _torch()
    with _on_stream(stream):
        # torch's caching allocator returns 512-byte aligned blocks; the ABI needs 256.
        return torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device)


def _workspace(workspace, entry: str, args, device, stream, tail: str = "too many keys or rows", zero_ok: bool = False,
               always: bool = False, status: int = errors.LSDSORT_ERR_TOO_LARGE):
    """The workspace step of every wrapper: the caller's ``workspace`` where one is given, else a temporary one of the size the
    unit's own ``entry`` (a ``*_workspace_bytes`` name) gives for ``args``, on ``device`` and under ``stream``.  A figure of 0 says
    that the library refuses the shape: ``LsdsortError(status, entry, tail)``, unless ``zero_ok`` (nothing will run).  ``always``:
    the figure is asked for, and checked, even when a workspace is given (the wide sorts)."""
    if workspace is not None and not always:
        return workspace
    nbytes = int(getattr(lib(), entry)(*args))
    if nbytes == 0 and not zero_ok:
        raise errors.LsdsortError(status, entry, tail)
    return workspace if workspace is not None else _temp_workspace(nbytes, device, stream)


def _ptr(t, live=True):
    """The pointer argument of an optional tensor: ``None`` (NULL) without one -- or, for the run units, without keys."""
    return t.data_ptr() if t is not None and live else None


def _check_fault(workspace, stream, entry: str = "lsdsort_check_device", *shape, quiet: bool = False) -> int:
    """Read back the fault word of the work queued in ``workspace`` and raise if it is set (synchronises ``stream``); ``quiet``:
    return the status instead.  ``entry`` and ``shape``: the wide sorts' check.  Callers ask only where kernels ran at all."""
    status = int(getattr(lib(), entry)(workspace.data_ptr(), *shape, _stream(stream)))
    if not quiet:
        check(status, entry)
    return status


def workspace_bytes(n: int, radix_bits: int = 8, pairs: int = False, algorithm: int = LSDSORT_ALGO_ONESWEEP) -> int:
    """Bytes of device workspace for a sort of up to ``n`` keys; ``pairs``: the number of payload arrays (False / True / 2 / 3).
    Keys only, default algorithm: the roomy size (``lsdsort_workspace_bytes_roomy``), which lets the hybrid form's half variant
    run at the sizes it exists for and is the plain size everywhere else."""
    if int(pairs) == 0 and algorithm == LSDSORT_ALGO_ONESWEEP:
        return int(lib().lsdsort_workspace_bytes_roomy(n, radix_bits))
    return int(lib().lsdsort_workspace_bytes_ex(n, radix_bits, int(pairs), algorithm))


def alloc_workspace(n: int, radix_bits: int = 8, pairs: int = False, algorithm: int = LSDSORT_ALGO_ONESWEEP,
                    device: str = "cuda", stream=None):
    """Workspace tensor for a sort of up to ``n`` keys with ``pairs`` payload arrays.  ``stream``: the stream the sort will
    run on when that is not torch's current stream (see ``_temp_workspace``)."""
    nbytes = workspace_bytes(n, radix_bits, pairs, algorithm)
    if nbytes == 0 and n > 0:
        raise errors.LsdsortError(errors.LSDSORT_ERR_INVALID_ARG, "lsdsort_workspace_bytes_ex", "bad (n, radix_bits)")
    return _temp_workspace(nbytes, device, stream)


def tile_keys(radix_bits: int) -> int:
    return int(lib().lsdsort_tile_keys(radix_bits))


def set_tile_config(radix_bits: int, config_id: int) -> None:
    check(lib().lsdsort_set_tile_config(radix_bits, config_id), "lsdsort_set_tile_config")


def set_xcd_chunk(chunk: int) -> None:
    """Consecutive tiles kept on one XCD by the rank-and-scatter kernel (0 = off; speed only)."""
    check(lib().lsdsort_set_xcd_chunk(chunk), "lsdsort_set_xcd_chunk")


def set_hybrid(on: bool) -> None:
    """The hybrid form of sorts of 2^25 .. 9.6e8 items with 8- or 4-bit digits (global passes on bits 16-31 + an LDS-resident local
    stage, decided on the device; ``lsdsort_set_hybrid``).  Default on; off = every digit through global memory, always."""
    check(lib().lsdsort_set_hybrid(1 if on else 0), "lsdsort_set_hybrid")


def set_half_hop(on: bool) -> None:
    """The hybrid form's half variant (``lsdsort_set_half_hop``): the second global pass writes and the local stage reads 16-bit
    halves, 24 B/key instead of 28, where the workspace has the roomy size.  Default on; off = never attempted."""
    check(lib().lsdsort_set_half_hop(1 if on else 0), "lsdsort_set_half_hop")


def set_small_sort(on: bool) -> None:
    """Sorts of up to 16384 items in one launch (``lsdsort_set_small_sort``).  Default on; off = the chained form at every size."""
    check(lib().lsdsort_set_small_sort(1 if on else 0), "lsdsort_set_small_sort")


def workspace_form(workspace, stream=None) -> int:
    """1 if the last sort queued in ``workspace`` ran the hybrid form, 0 if the ordinary passes (``lsdsort_workspace_form``)."""
    out = ctypes.c_int(0)
    check(lib().lsdsort_workspace_form(workspace.data_ptr(), _stream(stream), ctypes.byref(out)), "lsdsort_workspace_form")
    return out.value


def workspace_half(workspace, stream=None) -> int:
    """1 if the last sort queued in ``workspace`` ran the hybrid form's half variant (``lsdsort_workspace_half``)."""
    out = ctypes.c_int(0)
    check(lib().lsdsort_workspace_half(workspace.data_ptr(), _stream(stream), ctypes.byref(out)), "lsdsort_workspace_half")
    return out.value


def set_pass_skipping(on: bool) -> None:
    """Skip passes whose digit is the same for every key (decided on the device from the digit counts; default on)."""
    check(lib().lsdsort_set_pass_skipping(1 if on else 0), "lsdsort_set_pass_skipping")


def set_rank_method(method: int) -> None:
    """-1 auto, 0 peer-mask forms only, 2 returning-LDS-add wherever the device probe passed."""
    check(lib().lsdsort_set_rank_method(method), "lsdsort_set_rank_method")


def rank_method(radix_bits: int) -> int:
    m = lib().lsdsort_rank_method(radix_bits)
    if m < 0:
        check(m, "lsdsort_rank_method")
    return int(m)


# ------------------------------------------------------------------------------ device-resident sort
def GPULSDRadixSort(d_keys, r: int = 8, d_vals=None, algorithm: int = LSDSORT_ALGO_ONESWEEP, workspace=None,
                    stream=None, check_fault: bool = False):
    """Device-resident sort in place: the reference's ``GPULSDRadixSort(a, b, h, ...)`` (.cu:839).

    ``d_keys`` (and ``d_vals``) are int32 CUDA tensors of uint32 bit patterns; the result lands
    in ``d_keys`` like the reference's ``a``.  Stream-ordered, no synchronisation unless
    ``check_fault`` (then the workspace fault word is read back).
    """
    _dev(d_keys, "d_keys")
    n = d_keys.numel()
    pairs = d_vals is not None
    if pairs:
        _payload(d_vals, n)
    if workspace is None:
        workspace = alloc_workspace(n, r, pairs, algorithm, d_keys.device, stream)
    st = lib().lsdsort_u32_device_ex(d_keys.data_ptr(), d_vals.data_ptr() if pairs else None, workspace.data_ptr(),
                                     workspace.numel(), n, r, algorithm, _stream(stream))
    check(st, "lsdsort_u32_device_ex")
    if check_fault and n:
        _check_fault(workspace, stream)
    return d_keys if not pairs else (d_keys, d_vals)


def GPUSortMulti(d_keys, payloads, r: int = 8, workspace=None, stream=None, check_fault: bool = False):
    """Keys with one to three 32-bit payload arrays (``lsdsort_multi_u32_device``): every array in ``payloads`` (int32 CUDA
    tensors as long as ``d_keys``) is permuted exactly like the keys, stable by key.  In place."""
    _dev(d_keys, "d_keys")
    n = d_keys.numel()
    payloads = list(payloads)
    if not 1 <= len(payloads) <= 3:
        raise ValueError("one to three payload arrays")
    for i, v in enumerate(payloads):
        _payload(v, n, f"payloads[{i}]", what="payloads")
    if workspace is None:
        workspace = alloc_workspace(n, r, len(payloads), LSDSORT_ALGO_ONESWEEP, d_keys.device, stream)
    ptrs = (ctypes.c_void_p * len(payloads))(*[v.data_ptr() for v in payloads])
    check(lib().lsdsort_multi_u32_device(d_keys.data_ptr(), ptrs, len(payloads), workspace.data_ptr(), workspace.numel(), n, r,
                                         _stream(stream)), "lsdsort_multi_u32_device")
    if check_fault and n:
        _check_fault(workspace, stream)
    return d_keys, payloads


def GPUSortTyped(d_keys, key_type: str = "int32", descending: bool = False, d_vals=None, r: int = 8, workspace=None,
                 stream=None, check_fault: bool = False):
    """Device-resident sort of 32-bit keys of another type or order (``lsdsort_keys_device``): ``key_type`` in
    "uint32" / "int32" / "float32" says how the 32 bits of each element of ``d_keys`` (an int32 or float32 CUDA
    tensor) compare; float32 uses IEEE total order.  Stable with ``d_vals`` (int32 payloads).  In place."""
    torch = _torch()
    _dev(d_keys, "d_keys", (torch.int32, torch.float32))
    n = d_keys.numel()
    pairs = d_vals is not None
    if pairs:
        _payload(d_vals, n)
    code = _key_type(key_type, KEY_TYPES_32)
    if workspace is None:
        workspace = alloc_workspace(n, r, pairs, LSDSORT_ALGO_ONESWEEP, d_keys.device, stream)
    check(lib().lsdsort_keys_device(d_keys.data_ptr(), d_vals.data_ptr() if pairs else None, workspace.data_ptr(),
                                    workspace.numel(), n, r, code, int(bool(descending)), _stream(stream)),
          "lsdsort_keys_device")
    if check_fault and n:
        _check_fault(workspace, stream)
    return d_keys if not pairs else (d_keys, d_vals)


def segmented_workspace_bytes(n: int, num_segments: int, pairs: bool = False) -> int:
    """Bytes of device workspace ``GPUSortSegmented`` needs for up to ``n`` keys in up to ``num_segments`` segments."""
    return int(lib().lsdsort_segmented_workspace_bytes(n, num_segments, int(bool(pairs))))


def GPUSortSegmented(d_keys, d_offsets, d_vals=None, key_type: str = "uint32", descending: bool = False, workspace=None,
                     stream=None, check_fault: bool = False):
    """Sort every segment ``d_keys[d_offsets[s]:d_offsets[s + 1]]`` independently, in place, stable
    (``lsdsort_segmented_device``).  ``d_keys``: int32 or float32 CUDA tensor whose 32 bits compare as ``key_type``
    ("uint32" / "int32" / "float32", IEEE total order); ``d_offsets``: int32 CUDA tensor of num_segments + 1 ascending
    offsets (uint32 bit patterns); ``d_vals``: optional int32 payloads permuted with the keys.  Keys outside
    ``[d_offsets[0], d_offsets[-1])`` are left alone.  Malformed offsets are reported by the fault check
    (``check_fault=True`` raises)."""
    torch = _torch()
    _dev(d_keys, "d_keys", (torch.int32, torch.float32))
    _dev(d_offsets, "d_offsets")
    n = d_keys.numel()
    segs = max(d_offsets.numel() - 1, 0)
    pairs = d_vals is not None
    if pairs:
        _payload(d_vals, n)
    code = _key_type(key_type, KEY_TYPES_32)
    workspace = _workspace(workspace, "lsdsort_segmented_workspace_bytes", (n, segs, int(pairs)), d_keys.device, stream,
                           "too many keys or segments", zero_ok=not (n > 0 and segs > 0))
    check(lib().lsdsort_segmented_device(d_keys.data_ptr(), d_vals.data_ptr() if pairs else None, d_offsets.data_ptr(), segs, n,
                                         code, int(bool(descending)), workspace.data_ptr(), workspace.numel(), _stream(stream)),
          "lsdsort_segmented_device")
    if check_fault and n and segs:
        _check_fault(workspace, stream)
    return d_keys if not pairs else (d_keys, d_vals)


def sort_rows(x, descending: bool = False, return_indices: bool = False, stream=None):
    """``torch.sort(x, dim=-1, stable=True)`` for a contiguous 2-D int32 / float32 CUDA tensor: every row sorted by the
    library's segmented sort (float32 in IEEE total order: -0.0 before +0.0, NaNs by sign at the ends).  Returns the sorted
    copy, and with ``return_indices`` also the int64 positions within each row."""
    torch = _torch()
    _dev(x, "x", (torch.int32, torch.float32), dims=(2,), contiguous=False)
    rows, cols = x.shape
    key_type = "int32" if x.dtype == torch.int32 else "float32"
    with _on_stream(stream):
        out = x.contiguous().clone()
        offsets = torch.arange(0, rows + 1, dtype=torch.int64, device=x.device).mul_(cols).to(torch.int32)
        idx = torch.arange(cols, dtype=torch.int32, device=x.device).repeat(rows) if return_indices else None
        GPUSortSegmented(out.view(-1), offsets, d_vals=idx, key_type=key_type, descending=descending, stream=stream)
        if return_indices:
            return out, idx.view(rows, cols).to(torch.int64)
    return out


# ------------------------------------------------------------------------------ row selects, and what every row wrapper shares
def _rows_cols(d_keys):
    """(rows, cols) of a row entry's keys: a 1-D tensor is one row."""
    return (1, d_keys.shape[0]) if d_keys.dim() == 1 else d_keys.shape


def _keys32(d_keys):
    """The tensor check of the 32-bit row selects -> (rows, cols).  The key-type code is ``_select_code32``'s, a step of its
    own, because the three wrappers check k, the rank or the ranks between the two."""
    torch = _torch()
    _dev(d_keys, "d_keys", (torch.int32, torch.float32), dims=(1, 2))
    return _rows_cols(d_keys)


def _select_code32(d_keys, key_type: str, own_type_only: bool) -> int:
    """The key-type code of the 32-bit row selects.  ``own_type_only``: ``GPUKth`` and ``GPUKthMulti`` refuse a float32 tensor
    with another ``key_type``; ``GPUTopK`` takes it and compares the bits as it is told.  The difference is as old as the three
    entries and callers may rely on either side of it: it is kept here, not settled."""
    code = _key_type(key_type, KEY_TYPES_32)
    if own_type_only and d_keys.dtype == _torch().float32 and key_type != "float32":
        raise TypeError('a float32 tensor selects with key_type="float32" only (an int32 tensor holds any of the three bit patterns)')
    return code


def _select_outputs(d_keys, rows: int, tail: tuple, return_indices: bool, stream):
    """``(values, indices)`` of a row select: ``tail`` entries per row -- ``[rows] + tail``, for 1-D keys ``tail`` alone --, values
    in the keys' dtype, int32 positions or ``None``.  The outputs, like a temporary workspace, belong to the stream the kernels
    run on."""
    torch = _torch()
    shape = tail if d_keys.dim() == 1 else (rows,) + tail
    with _on_stream(stream):
        values = torch.empty(shape, dtype=d_keys.dtype, device=d_keys.device)
        indices = torch.empty(shape, dtype=torch.int32, device=d_keys.device) if return_indices else None
    return values, indices


def _ranks(ranks, cols: int) -> list:
    """The ranks of a multi-rank select: a sequence of 1 .. ``LSDSORT_KTH_MAX_RANKS`` ints, each within the row."""
    try:
        ranks = [int(r) for r in ranks]
    except TypeError:
        raise ValueError("ranks: a sequence of ints") from None
    if not 1 <= len(ranks) <= errors.LSDSORT_KTH_MAX_RANKS:
        raise ValueError(f"ranks: 1 .. {errors.LSDSORT_KTH_MAX_RANKS} of them, got {len(ranks)}")
    if not all(0 <= r < cols for r in ranks):
        raise ValueError("every rank must be within 0 .. the row length - 1")
    return ranks


class _Rows:
    """What every torch-shaped ``*_rows`` wrapper does with ``x``: the tensor check (one of ``dtypes``, any strides unless
    ``contiguous``), at least one dimension, and the rows of the last one -- ``cols``, the leading shape ``lead``, and the dtype's
    name as ``key_type``.  ``flat()`` is the ``[rows, cols]`` tensor a ``GPU*`` wrapper takes -- a copy where ``x`` is strided:
    call it under the stream --, ``restore`` gives a ``[rows, ...]`` result the leading shape back."""

    def __init__(self, x, dtypes, contiguous: bool = False):
        _dev(x, "x", dtypes, contiguous=contiguous)
        if x.dim() == 0:
            raise TypeError("x: at least one dimension")
        self.x, self.cols, self.lead, self.key_type = x, x.shape[-1], tuple(x.shape[:-1]), _dtype_name(x.dtype)

    @property
    def rows(self) -> int:
        return int(np.prod(self.lead, dtype=np.int64))

    def flat(self, copy: bool = True):
        return (self.x.contiguous() if copy else self.x).view(-1, self.cols)

    def restore(self, t, *tail):
        return t.view(self.lead + tail)


def topk_workspace_bytes(rows: int, cols: int, k: int) -> int:
    """Bytes of device workspace ``GPUTopK`` needs for the ``k`` best of each of ``rows`` rows of ``cols`` keys."""
    return int(lib().lsdsort_topk_workspace_bytes(rows, cols, k))


def GPUTopK(d_keys, k: int, key_type: str = "uint32", largest: bool = True, return_indices: bool = True, workspace=None,
            stream=None, check_fault: bool = False):
    """The ``k`` best keys of every row of ``d_keys`` (``lsdsort_topk_device``): a contiguous 1-D (one row) or 2-D int32 or
    float32 CUDA tensor whose 32 bits compare as ``key_type`` ("uint32" / "int32" / "float32", IEEE total order).  Returns
    ``(values, indices)`` -- ``[rows, k]`` (``[k]`` for 1-D input), best first, ``indices`` the int32 positions within the row,
    or ``None`` without ``return_indices`` -- exactly the first ``k`` columns of the rows' stable sort: equal keys in position
    order.  ``d_keys`` is only read.  Stream-ordered; the rows are not sorted (a radix select, then a sort of the winners)."""
    rows, cols = _keys32(d_keys)
    k = int(k)
    if not 0 <= k <= cols:
        raise ValueError("k must be within 0 .. the row length")
    code = _select_code32(d_keys, key_type, own_type_only=False)
    values, indices = _select_outputs(d_keys, rows, (k,), return_indices, stream)
    workspace = _workspace(workspace, "lsdsort_topk_workspace_bytes", (rows, cols, k), d_keys.device, stream)
    check(lib().lsdsort_topk_device(d_keys.data_ptr(), rows, cols, k, code, int(bool(largest)), values.data_ptr(), _ptr(indices),
                                    workspace.data_ptr(), workspace.numel(), _stream(stream)), "lsdsort_topk_device")
    if check_fault and rows and cols and k:
        _check_fault(workspace, stream)
    return values, indices


def _topk_rows(x, k, largest, stream, dtypes, select):
    """The body of ``topk_rows`` and ``topk16_rows``; ``select``: ``GPUTopK`` or ``GPUTopK16``."""
    r = _Rows(x, dtypes)
    with _on_stream(stream):
        values, indices = select(r.flat(), k, key_type=r.key_type, largest=largest, stream=stream)
        return r.restore(values, k), r.restore(indices, k).to(_torch().int64)


def _kthvalue_rows(x, k, stream, dtypes, select):
    """The body of ``kthvalue_rows`` and ``kthvalue16_rows``; ``select``: ``GPUKth`` or ``GPUKth16``."""
    r = _Rows(x, dtypes)
    k = int(k)
    if not 1 <= k <= r.cols:
        raise ValueError("k must be within 1 .. the row length")
    with _on_stream(stream):
        values, indices = select(r.flat(), k - 1, key_type=r.key_type, stream=stream)
        return r.restore(values), r.restore(indices).to(_torch().int64)


def topk_rows(x, k: int, largest: bool = True, stream=None):
    """``torch.topk(x, k, dim=-1, largest=largest, sorted=True)`` for a contiguous int32 / float32 CUDA tensor of one or more
    dimensions: ``(values, int64 indices)``.  float32 follows IEEE total order, not torch's: NaNs by sign at the two ends
    (+NaN above +inf, -NaN below -inf) and -0.0 below +0.0.  Among equal keys the lower position comes first, always."""
    torch = _torch()
    return _topk_rows(x, k, largest, stream, (torch.int32, torch.float32), GPUTopK)


def kth_workspace_bytes(rows: int, cols: int) -> int:
    """Bytes of device workspace ``GPUKth`` needs for one rank of each of ``rows`` rows of ``cols`` keys (whatever the rank)."""
    return int(lib().lsdsort_kth_workspace_bytes(rows, cols))


def GPUKth(d_keys, rank: int, key_type: str = "uint32", largest: bool = False, return_indices: bool = True, workspace=None,
           stream=None, check_fault: bool = False):
    """The key at 0-based ``rank`` of every row's stable sort (``lsdsort_kth_device``): ``d_keys`` is a contiguous 1-D (one row) or
    2-D int32 or float32 CUDA tensor whose 32 bits compare as ``key_type`` ("uint32" / "int32" / "float32", IEEE total order);
    ``largest`` counts the rank from the largest key down.  Returns ``(values, indices)`` -- ``[rows]`` (0-D for 1-D input),
    ``indices`` the int32 position within the row of that very item, or ``None`` without ``return_indices`` -- exactly column
    ``rank`` of ``GPUTopK(d_keys, rank + 1, ...)``: among equal keys the stable sort's position, on every run.  ``d_keys`` is only
    read.  A float32 tensor goes with ``key_type="float32"`` only; an int32 tensor holds the bit patterns of any of the three.
    Stream-ordered; the rows are not sorted and no winner is written (a radix select, then a locate)."""
    rows, cols = _keys32(d_keys)
    rank = int(rank)
    if not 0 <= rank < cols:
        raise ValueError("rank must be within 0 .. the row length - 1")
    code = _select_code32(d_keys, key_type, own_type_only=True)
    values, indices = _select_outputs(d_keys, rows, (), return_indices, stream)
    workspace = _workspace(workspace, "lsdsort_kth_workspace_bytes", (rows, cols), d_keys.device, stream)
    check(lib().lsdsort_kth_device(d_keys.data_ptr(), rows, cols, rank, code, int(bool(largest)), values.data_ptr(), _ptr(indices),
                                   workspace.data_ptr(), workspace.numel(), _stream(stream)), "lsdsort_kth_device")
    if check_fault and rows and cols:
        _check_fault(workspace, stream)
    return values, indices


def kthvalue_rows(x, k: int, stream=None):
    """``torch.kthvalue(x, k, dim=-1)`` for a contiguous int32 / float32 CUDA tensor of one or more dimensions: ``k`` is 1-based,
    the k-th smallest of every row -> ``(values, int64 indices)`` of the leading shape.  float32 follows IEEE total order, not
    torch's: a row with NaNs does NOT propagate NaN as ``torch.kthvalue`` / ``torch.median`` do -- NaNs sort by sign at the two
    ends (+NaN above +inf, -NaN below -inf), and -0.0 below +0.0.  The index is the stable sort's (among equal keys the one the
    stable sort puts at that rank), where torch leaves it unspecified among ties."""
    torch = _torch()
    return _kthvalue_rows(x, k, stream, (torch.int32, torch.float32), GPUKth)


def median_rows(x, stream=None):
    """``torch.median(x, dim=-1)`` for a contiguous int32 / float32 CUDA tensor of one or more dimensions: ``kthvalue_rows`` at
    rank ``(cols - 1) // 2``, the lower median torch returns -> ``(values, int64 indices)``.  float32 follows IEEE total order: a
    row with NaNs does NOT propagate NaN as ``torch.median`` does (NaNs sort by sign at the two ends).  The index is the stable
    sort's, where torch leaves it unspecified among ties."""
    torch = _torch()
    _dev(x, "x", (torch.int32, torch.float32), contiguous=False)
    if x.dim() == 0 or x.shape[-1] == 0:
        raise ValueError("x: at least one dimension, and a last one that is not empty")
    return kthvalue_rows(x, (x.shape[-1] - 1) // 2 + 1, stream=stream)


def kth_multi_workspace_bytes(rows: int, cols: int, num_ranks: int) -> int:
    """Bytes of device workspace ``GPUKthMulti`` needs for ``num_ranks`` ranks of each of ``rows`` rows of ``cols`` keys (whatever
    the ranks)."""
    return int(lib().lsdsort_kth_multi_workspace_bytes(rows, cols, num_ranks))


def GPUKthMulti(d_keys, ranks, key_type: str = "uint32", largest: bool = False, return_indices: bool = True, workspace=None,
                stream=None, check_fault: bool = False):
    """The keys at several 0-based ``ranks`` of every row's stable sort, in one call (``lsdsort_kth_multi_device``): ``GPUKth``
    argument for argument, with a sequence of 1 .. ``LSDSORT_KTH_MAX_RANKS`` ranks in ``0 .. cols - 1`` -- in any order, repeats
    allowed -- where it has one.  Returns ``(values, indices)`` of shape ``[rows, m]`` (``[m]`` for 1-D input): column ``j`` is
    exactly ``GPUKth(d_keys, ranks[j], ...)``, values and int32 positions bit for bit; ``indices`` is ``None`` without
    ``return_indices``.  ``d_keys`` is only read, and read once for all ranks where ``GPUKth`` reads it once per rank.  The ranks
    are host values: they are fixed in a captured graph."""
    rows, cols = _keys32(d_keys)
    ranks = _ranks(ranks, cols)
    code = _select_code32(d_keys, key_type, own_type_only=True)
    m = len(ranks)
    values, indices = _select_outputs(d_keys, rows, (m,), return_indices, stream)
    workspace = _workspace(workspace, "lsdsort_kth_multi_workspace_bytes", (rows, cols, m), d_keys.device, stream)
    check(lib().lsdsort_kth_multi_device(d_keys.data_ptr(), rows, cols, (ctypes.c_size_t * m)(*ranks), m, code, int(bool(largest)),
                                         values.data_ptr(), _ptr(indices), workspace.data_ptr(), workspace.numel(), _stream(stream)),
          "lsdsort_kth_multi_device")
    if check_fault and rows and cols:
        _check_fault(workspace, stream)
    return values, indices


QUANTILE_MODES = ("linear", "lower", "higher", "midpoint", "nearest")


def quantile_ranks(q, cols: int, interpolation: str = "linear"):
    """The host half of ``quantile_rows``, torch.quantile's own arithmetic: ``q`` (a float, a sequence, or a 0-D or 1-D tensor
    with values in [0, 1]) and the row length -> ``(below, above, weights, scalar)``.  ``below`` and ``above`` are lists of the
    order statistics every quantile is made of, ``weights`` a float32 CPU tensor, ``scalar`` whether ``q`` had no dimension:
    quantile i is ``torch.lerp(sorted[below[i]], sorted[above[i]], weights[i])``; for ``lower`` / ``higher`` / ``nearest`` it is
    ``sorted[below[i]]`` itself, and ``above`` and ``weights`` are ``None``.
    ``ranks = q.to(float32) * (cols - 1)``, in float32; ``lower`` floors it, ``higher`` takes the ceiling, ``nearest`` rounds half
    to even; ``linear`` takes floor and ceiling with the weight ``ranks - floor``, ``midpoint`` the same two with the weight 0.5.
    Needs no device and no library."""
    torch = _torch()
    if interpolation not in QUANTILE_MODES:
        raise ValueError("interpolation: " + " or ".join(f'"{m}"' for m in QUANTILE_MODES) + f", got {interpolation!r}")
    cols = int(cols)
    if cols < 1:
        raise ValueError("x: a last dimension that is not empty")
    qt = q.detach().cpu().to(torch.float32) if isinstance(q, torch.Tensor) else torch.as_tensor(q, dtype=torch.float32)
    if qt.dim() > 1:
        raise ValueError("q: a float, a sequence of floats, or a 0-D or 1-D tensor")
    scalar = qt.dim() == 0
    qt = qt.reshape(-1)
    if not bool(((qt >= 0) & (qt <= 1)).all()):
        raise ValueError("q: values within [0, 1]")
    ranks = qt * (cols - 1)
    if interpolation == "lower":
        ranks = ranks.floor()
    elif interpolation == "higher":
        ranks = ranks.ceil()
    elif interpolation == "nearest":
        ranks = ranks.round()
    below = ranks.floor()
    if interpolation not in ("linear", "midpoint"):
        return below.to(torch.int64).tolist(), None, None, scalar
    weights = torch.full_like(ranks, 0.5) if interpolation == "midpoint" else ranks - below
    return below.to(torch.int64).tolist(), ranks.ceil().to(torch.int64).tolist(), weights, scalar


def quantile_rows(x, q, interpolation: str = "linear", stream=None):
    """``torch.quantile(x, q, dim=-1, keepdim=False, interpolation=...)`` for a float32 CUDA tensor of one or more dimensions,
    without sorting a row: the order statistics the quantiles are made of come from ``GPUKthMulti``.  ``q`` is a float, a sequence,
    or a 0-D or 1-D tensor with values in [0, 1]; it is brought to the host, because ranks are host arguments.  The result has
    torch's shape: the leading shape of ``x`` for a scalar ``q``, ``(len(q),)`` + the leading shape for a 1-D ``q``.
    The arithmetic is torch's own (``quantile_ranks``): ``ranks = q.to(float32) * (cols - 1)`` in float32; ``lower`` takes the
    value at the floor, ``higher`` at the ceiling, ``nearest`` at ``round`` (half to even); ``linear`` is
    ``torch.lerp(v[floor], v[ceil], ranks - floor)`` and ``midpoint`` ``torch.lerp(v[floor], v[ceil], 0.5)``.  The distinct integer
    ranks of a call are de-duplicated and selected in groups of at most ``LSDSORT_KTH_MAX_RANKS``: more distinct ranks than that
    mean more than one read of ``x``.
    float32 follows IEEE total order, not torch's: a row with NaNs does NOT propagate NaN as ``torch.quantile`` does -- NaNs sort
    by sign at the two ends (+NaN above +inf, -NaN below -inf), and -0.0 below +0.0."""
    def select(flat, ranks):
        return GPUKthMulti(flat, ranks, key_type="float32", return_indices=False, stream=stream)[0]

    return _quantile_of(x, (_torch().float32,), q, interpolation, stream, select)


def _quantile_of(x, dtypes, q, interpolation, stream, select):
    """What ``quantile_rows`` and ``quantile16_rows`` share: ``select(flat, ranks)`` -> the float32 ``[rows, len(ranks)]`` order
    statistics of at most ``LSDSORT_KTH_MAX_RANKS`` distinct ranks; the rest is ``quantile_ranks`` and torch's own arithmetic."""
    torch = _torch()
    r = _Rows(x, dtypes)
    below, above, weights, scalar = quantile_ranks(q, r.cols, interpolation)
    distinct = sorted(set(below) | set(above or ()))
    slot = {rank: i for i, rank in enumerate(distinct)}
    group = errors.LSDSORT_KTH_MAX_RANKS
    with _on_stream(stream):
        flat = r.flat()
        parts = [select(flat, distinct[at:at + group]) for at in range(0, len(distinct), group)]
        stats = torch.cat(parts, dim=1) if parts else flat.new_empty((flat.shape[0], 0), dtype=torch.float32)   # [rows, distinct ranks]

        def take(ranks):
            return stats.index_select(1, torch.tensor([slot[r] for r in ranks], dtype=torch.int64).to(x.device, non_blocking=True))

        values = take(below)
        if above is not None:
            values = torch.lerp(values, take(above), weights.to(x.device, non_blocking=True))
        values = r.restore(values, len(below)).movedim(-1, 0)
        return values[0] if scalar else values


def GPUSortWide(d_keys, d_vals=None, r: int = 8, workspace=None, stream=None, check_fault: bool = False, key_type: str = "uint64",
                descending: bool = False):
    """64-bit keys and / or 64-bit payloads, in place (``lsdsort_keys64_device`` / ``lsdsort_records_device``).
    ``d_keys``: int64 CUDA tensor whose 64 bits compare as ``key_type`` ("uint64", the default: uint64 bit patterns, so negative
    int64 values sort AFTER the positive ones; "int64"; "float64": the bit patterns of doubles), a float64 tensor with ``key_type="float64"`` (IEEE total
    order: NaNs by sign at the two ends, -0.0 below +0.0), or int32 (uint32 bit patterns; ascending only); ``d_vals``: None (64-bit keys only),
    int32 or int64.  The 32/32 combination is ``GPULSDRadixSort``.  Stable by key, ``descending`` too."""
    torch = _torch()
    code = _key_type(key_type, KEY_TYPES_64)
    _dev(d_keys, "d_keys", (torch.int32, torch.int64, torch.float64))
    if d_keys.dtype == torch.float64 and key_type != "float64":
        raise TypeError('a float64 tensor sorts with key_type="float64" only')
    kb = 32 if d_keys.dtype == torch.int32 else 64
    vb = 0
    if d_vals is not None:
        _payload(d_vals, d_keys.numel(), dtypes=(torch.int32, torch.int64))
        vb = 32 if d_vals.dtype == torch.int32 else 64
    if (kb, vb) in ((32, 0), (32, 32)):
        raise ValueError("32-bit keys with no or 32-bit payloads: use GPULSDRadixSort")
    if kb == 32 and (key_type != "uint64" or descending):
        raise ValueError("32-bit keys with 64-bit payloads sort as uint32, ascending, only")
    n = d_keys.numel()
    workspace = _workspace(workspace, "lsdsort_wide_workspace_bytes", (n, r, kb, vb), d_keys.device, stream, "bad (n, radix_bits)",
                           always=True, status=errors.LSDSORT_ERR_INVALID_ARG)
    if kb == 64:
        st = lib().lsdsort_keys64_device(d_keys.data_ptr(), d_vals.data_ptr() if vb else None, vb, workspace.data_ptr(),
                                         workspace.numel(), n, r, code, int(bool(descending)), _stream(stream))
        check(st, "lsdsort_keys64_device")
    else:
        st = lib().lsdsort_records_device(d_keys.data_ptr(), d_vals.data_ptr(), kb, vb, workspace.data_ptr(), workspace.numel(), n, r,
                                          _stream(stream))
        check(st, "lsdsort_records_device")
    if check_fault and n:
        _check_fault(workspace, stream, "lsdsort_wide_check_device", n, r, kb, vb)
    return d_keys if d_vals is None else (d_keys, d_vals)


def sort64(x, descending: bool = False, return_indices: bool = False, stream=None):
    """``torch.sort(x, stable=True, descending=descending)`` for a 1-D int64 / float64 CUDA tensor, the 64-bit counterpart of
    ``sort_rows``: returns the sorted copy, and with ``return_indices`` also the int64 positions (a 64/32 records sort with the
    positions as payload, so equal keys keep their input order in either direction).  float64 follows IEEE total order, not
    torch's: NaNs by sign at the two ends (+NaN above +inf, -NaN below -inf) and -0.0 below +0.0."""
    torch = _torch()
    return _sort_1d(x, (torch.int64, torch.float64), return_indices, stream,
                    lambda out, idx, key_type: GPUSortWide(out, idx, key_type=key_type, descending=descending, stream=stream))


def _sort_1d(x, dtypes, return_indices: bool, stream, sort):
    """The body of ``sort64`` and ``sort16``: ``sort(out, idx, key_type)`` sorts the contiguous copy ``out`` of ``x`` in place as
    the dtype's own key type, with the int32 positions ``idx`` (or ``None``) as its payload."""
    torch = _torch()
    _dev(x, "x", dtypes, dims=(1,), contiguous=False)
    with _on_stream(stream):
        out = x.clone(memory_format=torch.contiguous_format)
        idx = torch.arange(x.numel(), dtype=torch.int32, device=x.device) if return_indices else None
        sort(out, idx, _dtype_name(x.dtype))
        if return_indices:
            return out, idx.to(torch.int64)
    return out


# ------------------------------------------------------------------------------ 16-bit keys
_FITS16 = {"int16": ("uint16", "int16"), "float16": ("float16",), "bfloat16": ("bfloat16",)}   # dtype -> the key types it pairs with


def _keys16(d_keys, key_type: str, verb: str = "selects", dims=(1, 2)):
    """The tensor and key-type checks of every 16-bit entry -> (code, rows, cols); ``verb``: what the message says the tensor
    does with its key type; ``dims``: the dimensions the entry takes (the plain sort: one)."""
    torch = _torch()
    _dev(d_keys, "d_keys", (torch.int16, torch.float16, torch.bfloat16), dims=dims)
    code = _key_type(key_type, KEY_TYPES_16)
    fits = _FITS16[_dtype_name(d_keys.dtype)]
    if key_type not in fits:
        raise TypeError(f"a {_dtype_name(d_keys.dtype)} tensor {verb} with key_type " + " or ".join(f'"{k}"' for k in fits))
    rows, cols = _rows_cols(d_keys)
    return code, rows, cols


def _logits16(d_keys, key_type: str, verb: str):
    """``_keys16`` for the units that weigh logits (the top-p filter, the draw, the log-probabilities): the float types only."""
    torch = _torch()
    _dev(d_keys, "d_keys", (torch.float16, torch.bfloat16), dims=(1, 2))
    if key_type not in ("float16", "bfloat16"):
        raise ValueError(f'key_type: "float16" or "bfloat16", got {key_type!r}')
    return _keys16(d_keys, key_type, verb)


def _per_row(t, name: str, rows: int, dtype, dims=None, optional: bool = False):
    """A per-row device argument or output: a contiguous CUDA tensor of ``dtype`` with one entry per row (``dims``: of that many
    dimensions); ``optional``: or ``None``."""
    if t is None and optional:
        return None
    _dev(t, name, (dtype,), dims=dims)
    if t.numel() != rows:
        raise ValueError(f"{name}: one entry per row ({rows}), got {t.numel()}")
    return t


def _row_out(out, d_keys):
    """``out`` of the entries that write rows like their keys': ``None``, or a contiguous CUDA tensor of the keys' dtype and shape."""
    if out is not None:
        _dev(out, "out", (d_keys.dtype,), dims=(d_keys.dim(),))
        if out.shape != d_keys.shape:
            raise ValueError("out: the shape of d_keys")
    return out


def _fill16(fill, key_type: str, largest: bool) -> int:
    """``fill`` of the two filters: a 16-bit word; ``None``: the value that ranks last in the requested order."""
    if fill is None:
        fill = _worst_bits16(key_type, largest)
    if isinstance(fill, bool) or not isinstance(fill, int) or not 0 <= fill <= 0xFFFF:
        raise ValueError("fill: a 16-bit word, an int within 0 .. 0xFFFF")
    return fill


def keys16_workspace_bytes(n: int, pairs: bool = False) -> int:
    """Bytes of device workspace ``GPUSort16`` needs for up to ``n`` 16-bit keys (``pairs``: with 32-bit payloads); the figure
    covers both routes."""
    return int(lib().lsdsort_keys16_workspace_bytes(n, int(bool(pairs))))


def set_keys16_route(route: int) -> None:
    """How ``GPUSort16`` sorts keys without payloads: -1 by size (default), 0 always the widen route (map to uint32, the ordinary
    sort, narrow), 1 always the count route (count the 65536 values, scan, fill).  Payloads always take the widen route."""
    check(lib().lsdsort_set_keys16_route(route), "lsdsort_set_keys16_route")


def GPUSort16(d_keys, key_type: str = "int16", descending: bool = False, d_vals=None, workspace=None, stream=None,
              check_fault: bool = False):
    """Device-resident sort of 16-bit keys, in place (``lsdsort_keys16_device``).  ``d_keys``: a contiguous 1-D int16, float16 or
    bfloat16 CUDA tensor whose 16 bits compare as ``key_type``: "uint16" / "int16" for an int16 tensor ("uint16" sorts its bit
    patterns), "float16" / "bfloat16" for the tensor of that dtype (IEEE total order: NaNs by sign at the two ends, -0.0 below
    +0.0).  ``d_vals``: optional int32 payloads permuted with the keys, stable in either direction."""
    code, _, n = _keys16(d_keys, key_type, "sorts", dims=(1,))
    pairs = d_vals is not None
    if pairs:
        _payload(d_vals, n)
    workspace = _workspace(workspace, "lsdsort_keys16_workspace_bytes", (n, int(pairs)), d_keys.device, stream, "too many keys")
    check(lib().lsdsort_keys16_device(d_keys.data_ptr(), _ptr(d_vals), workspace.data_ptr(), workspace.numel(), n, code,
                                      int(bool(descending)), _stream(stream)), "lsdsort_keys16_device")
    if check_fault and n:
        _check_fault(workspace, stream, "lsdsort_keys16_check_device", n, int(pairs))
    return d_keys if not pairs else (d_keys, d_vals)


def sort16(x, descending: bool = False, return_indices: bool = False, stream=None):
    """``torch.sort(x, stable=True, descending=descending)`` for a 1-D int16 / float16 / bfloat16 CUDA tensor, the 16-bit
    counterpart of ``sort64``: returns the sorted copy (large sorts by counting the 65536 values: no key is moved), and with
    ``return_indices`` also the int64 positions (the positions ride as payloads, so equal keys keep their input order in either
    direction).  The float types follow IEEE total order, not torch's: NaNs by sign at the two ends and -0.0 below +0.0."""
    torch = _torch()
    return _sort_1d(x, (torch.int16, torch.float16, torch.bfloat16), return_indices, stream,
                    lambda out, idx, key_type: GPUSort16(out, key_type=key_type, descending=descending, d_vals=idx, stream=stream))


def topk16_workspace_bytes(rows: int, cols: int, k: int) -> int:
    """Bytes of device workspace ``GPUTopK16`` needs for the ``k`` best of each of ``rows`` rows of ``cols`` 16-bit keys."""
    return int(lib().lsdsort_topk16_workspace_bytes(rows, cols, k))


def GPUTopK16(d_keys, k: int, key_type: str = "int16", largest: bool = True, return_indices: bool = True, workspace=None,
              stream=None, check_fault: bool = False):
    """The ``k`` best keys of every row of ``d_keys`` (``lsdsort_topk16_device``): a contiguous 1-D (one row) or 2-D int16, float16
    or bfloat16 CUDA tensor whose 16 bits compare as ``key_type``, paired with the dtype as in ``GPUSort16``: "uint16" / "int16" for
    an int16 tensor, "float16" / "bfloat16" for the tensor of that dtype (IEEE total order).  Returns ``(values, indices)`` --
    ``[rows, k]`` (``[k]`` for 1-D input), best first, ``values`` in the input's dtype, ``indices`` the int32 positions within the
    row, or ``None`` without ``return_indices`` -- exactly the first ``k`` columns of the rows' stable sort: equal keys in position
    order.  ``d_keys`` is only read.  Stream-ordered; the rows are not sorted (a radix select of at most two digit levels, then a
    sort of the winners)."""
    code, rows, cols = _keys16(d_keys, key_type)
    k = int(k)
    if not 0 <= k <= cols:
        raise ValueError("k must be within 0 .. the row length")
    values, indices = _select_outputs(d_keys, rows, (k,), return_indices, stream)
    workspace = _workspace(workspace, "lsdsort_topk16_workspace_bytes", (rows, cols, k), d_keys.device, stream)
    check(lib().lsdsort_topk16_device(d_keys.data_ptr(), rows, cols, k, code, int(bool(largest)), values.data_ptr(), _ptr(indices),
                                      workspace.data_ptr(), workspace.numel(), _stream(stream)), "lsdsort_topk16_device")
    if check_fault and rows and cols and k:
        _check_fault(workspace, stream)
    return values, indices


def topk16_rows(x, k: int, largest: bool = True, stream=None):
    """``torch.topk(x, k, dim=-1, largest=largest, sorted=True)`` for a contiguous int16 / float16 / bfloat16 CUDA tensor of one or
    more dimensions, the 16-bit counterpart of ``topk_rows``: ``(values, int64 indices)``.  The float types follow IEEE total
    order, not torch's: NaNs by sign at the two ends (+NaN above +inf, -NaN below -inf) and -0.0 below +0.0.  Among equal keys the
    lower position comes first, always."""
    torch = _torch()
    return _topk_rows(x, k, largest, stream, (torch.int16, torch.float16, torch.bfloat16), GPUTopK16)


def kth16_workspace_bytes(rows: int, cols: int) -> int:
    """Bytes of device workspace ``GPUKth16`` needs for one rank of each of ``rows`` rows of ``cols`` 16-bit keys (whatever the
    rank, with or without indices)."""
    return int(lib().lsdsort_kth16_workspace_bytes(rows, cols))


def GPUKth16(d_keys, rank: int, key_type: str = "int16", largest: bool = False, return_indices: bool = True, workspace=None,
             stream=None, check_fault: bool = False):
    """The key at 0-based ``rank`` of every row's stable sort (``lsdsort_kth16_device``): ``d_keys`` is a contiguous 1-D (one row)
    or 2-D int16, float16 or bfloat16 CUDA tensor whose 16 bits compare as ``key_type``, paired with the dtype as in ``GPUTopK16``:
    "uint16" / "int16" for an int16 tensor, "float16" / "bfloat16" for the tensor of that dtype (IEEE total order); ``largest``
    counts the rank from the largest key down.  Returns ``(values, indices)`` -- ``[rows]`` (0-D for 1-D input), ``values`` in the
    input's dtype, ``indices`` the int32 position within the row of that very item, or ``None`` without ``return_indices`` --
    exactly column ``rank`` of ``GPUTopK16(d_keys, rank + 1, ...)``: among equal keys the stable sort's position, on every run.
    ``d_keys`` is only read and never widened.  Stream-ordered; the rows are not sorted and no winner is written (a radix select of
    at most two digit levels, then a locate; without indices a row above 16384 keys needs no locate)."""
    code, rows, cols = _keys16(d_keys, key_type)
    rank = int(rank)
    if not 0 <= rank < cols:
        raise ValueError("rank must be within 0 .. the row length - 1")
    values, indices = _select_outputs(d_keys, rows, (), return_indices, stream)
    workspace = _workspace(workspace, "lsdsort_kth16_workspace_bytes", (rows, cols), d_keys.device, stream)
    check(lib().lsdsort_kth16_device(d_keys.data_ptr(), rows, cols, rank, code, int(bool(largest)), values.data_ptr(), _ptr(indices),
                                     workspace.data_ptr(), workspace.numel(), _stream(stream)), "lsdsort_kth16_device")
    if check_fault and rows and cols:
        _check_fault(workspace, stream)
    return values, indices


def kthvalue16_rows(x, k: int, stream=None):
    """``torch.kthvalue(x, k, dim=-1)`` for an int16 / float16 / bfloat16 CUDA tensor of one or more dimensions, the 16-bit
    counterpart of ``kthvalue_rows``: ``k`` is 1-based, the k-th smallest of every row -> ``(values, int64 indices)`` of the leading
    shape.  The float types follow IEEE total order, not torch's: a row with NaNs does NOT propagate NaN as ``torch.kthvalue`` /
    ``torch.median`` do -- NaNs sort by sign at the two ends (+NaN above +inf, -NaN below -inf), and -0.0 below +0.0.  The index is
    the stable sort's (among equal keys the one the stable sort puts at that rank), where torch leaves it unspecified among ties."""
    torch = _torch()
    return _kthvalue_rows(x, k, stream, (torch.int16, torch.float16, torch.bfloat16), GPUKth16)


def median16_rows(x, stream=None):
    """``torch.median(x, dim=-1)`` for an int16 / float16 / bfloat16 CUDA tensor of one or more dimensions: ``kthvalue16_rows`` at
    rank ``(cols - 1) // 2``, the lower median torch returns -> ``(values, int64 indices)``.  The float types follow IEEE total
    order: a row with NaNs does NOT propagate NaN as ``torch.median`` does (NaNs sort by sign at the two ends), and -0.0 lies below
    +0.0.  The index is the stable sort's, where torch leaves it unspecified among ties."""
    torch = _torch()
    _dev(x, "x", (torch.int16, torch.float16, torch.bfloat16), contiguous=False)
    if x.dim() == 0 or x.shape[-1] == 0:
        raise ValueError("x: at least one dimension, and a last one that is not empty")
    return kthvalue16_rows(x, (x.shape[-1] - 1) // 2 + 1, stream=stream)


def kth16_multi_workspace_bytes(rows: int, cols: int, num_ranks: int) -> int:
    """Bytes of device workspace ``GPUKth16Multi`` needs for ``num_ranks`` ranks of each of ``rows`` rows of ``cols`` 16-bit keys
    (whatever the ranks, with or without indices)."""
    return int(lib().lsdsort_kth16_multi_workspace_bytes(rows, cols, num_ranks))


def GPUKth16Multi(d_keys, ranks, key_type: str = "int16", largest: bool = False, return_indices: bool = True, workspace=None,
                  stream=None, check_fault: bool = False):
    """The 16-bit keys at several 0-based ``ranks`` of every row's stable sort, in one call (``lsdsort_kth16_multi_device``):
    ``GPUKth16`` argument for argument -- the same tensors, and the same pairing of dtype and ``key_type`` -- with a sequence of
    1 .. ``LSDSORT_KTH_MAX_RANKS`` ranks in ``0 .. cols - 1``, in any order, repeats allowed, where it has one.  Returns
    ``(values, indices)`` of shape ``[rows, m]`` (``[m]`` for 1-D input): column ``j`` is exactly ``GPUKth16(d_keys, ranks[j], ...)``,
    values in the input's dtype and int32 positions bit for bit; ``indices`` is ``None`` without ``return_indices``.  ``d_keys`` is
    only read and never widened, and read once for all ranks where ``GPUKth16`` reads it once per rank; without indices a row above
    16384 keys is read twice, whatever the number of ranks.  The ranks are host values: they are fixed in a captured graph."""
    code, rows, cols = _keys16(d_keys, key_type)
    ranks = _ranks(ranks, cols)
    m = len(ranks)
    values, indices = _select_outputs(d_keys, rows, (m,), return_indices, stream)
    workspace = _workspace(workspace, "lsdsort_kth16_multi_workspace_bytes", (rows, cols, m), d_keys.device, stream)
    check(lib().lsdsort_kth16_multi_device(d_keys.data_ptr(), rows, cols, (ctypes.c_size_t * m)(*ranks), m, code, int(bool(largest)),
                                           values.data_ptr(), _ptr(indices), workspace.data_ptr(), workspace.numel(), _stream(stream)),
          "lsdsort_kth16_multi_device")
    if check_fault and rows and cols:
        _check_fault(workspace, stream)
    return values, indices


def quantile16_rows(x, q, interpolation: str = "linear", stream=None):
    """``torch.quantile(x.float(), q, dim=-1, keepdim=False, interpolation=...)`` for a float16 / bfloat16 CUDA tensor of one or
    more dimensions -- which ``torch.quantile`` itself refuses -- without widening ``x`` and without sorting a row: the 16-bit
    counterpart of ``quantile_rows``.  The result is **float32**, in torch's shapes.  ``quantile_ranks`` gives the order statistics
    the quantiles are made of; the distinct ones come from ``GPUKth16Multi(..., return_indices=False)`` in groups of at most
    ``LSDSORT_KTH_MAX_RANKS`` (two reads of a long row per group), are converted with ``.float()`` -- exact -- and go through
    ``quantile_rows``' own ``index_select`` / ``torch.lerp``.
    As in ``kthvalue16_rows`` the float types follow IEEE total order, not torch's: a row with NaNs does NOT propagate NaN as
    ``torch.quantile`` does -- NaNs sort by sign at the two ends (+NaN above +inf, -NaN below -inf), and -0.0 below +0.0."""
    torch = _torch()

    def select(flat, ranks):
        return GPUKth16Multi(flat, ranks, key_type=_dtype_name(flat.dtype), return_indices=False, stream=stream)[0].float()

    return _quantile_of(x, (torch.float16, torch.bfloat16), q, interpolation, stream, select)


def kth16_perrow_workspace_bytes(rows: int, cols: int) -> int:
    """Bytes of device workspace ``GPUKth16PerRow`` needs for ``rows`` rows of ``cols`` 16-bit keys (whatever the ranks, with or
    without indices)."""
    return int(lib().lsdsort_kth16_perrow_workspace_bytes(rows, cols))


def GPUKth16PerRow(d_keys, d_ranks, key_type: str = "int16", largest: bool = False, return_indices: bool = True, workspace=None,
                   stream=None, check_fault: bool = False):
    """``GPUKth16`` with a rank of its own for every row, read on the device (``lsdsort_kth16_perrow_device``): ``d_ranks`` is a
    contiguous int32 CUDA tensor with one 0-based rank per row.  Returns ``(values, indices)`` as ``GPUKth16`` does, and row ``r``
    holds exactly what ``GPUKth16(d_keys, d_ranks[r], ...)`` gives for it, values and int32 positions bit for bit.  The host never
    reads ``d_ranks``: a captured graph follows its contents from replay to replay, and no launch depends on them.  A row whose rank
    is outside ``0 .. cols - 1`` (as uint32) has nothing stored for it -- its slots of the returned tensors are uninitialised --, the
    other rows are right, and ``check_fault=True`` raises ``LsdsortError`` (``LSDSORT_ERR_DEVICE_FAULT``: bit 4096 of the workspace's
    first word)."""
    code, rows, cols = _keys16(d_keys, key_type)
    _per_row(d_ranks, "d_ranks", rows, _torch().int32)
    values, indices = _select_outputs(d_keys, rows, (), return_indices, stream)
    workspace = _workspace(workspace, "lsdsort_kth16_perrow_workspace_bytes", (rows, cols), d_keys.device, stream)
    check(lib().lsdsort_kth16_perrow_device(d_keys.data_ptr(), rows, cols, d_ranks.data_ptr(), code, int(bool(largest)),
                                            values.data_ptr(), _ptr(indices), workspace.data_ptr(), workspace.numel(), _stream(stream)),
          "lsdsort_kth16_perrow_device")
    if check_fault and rows and cols:
        _check_fault(workspace, stream)
    return values, indices


def topk16_filter_workspace_bytes(rows: int, cols: int) -> int:
    """Bytes of device workspace ``GPUTopK16Filter`` needs for ``rows`` rows of ``cols`` 16-bit keys (whatever the k's)."""
    return int(lib().lsdsort_topk16_filter_workspace_bytes(rows, cols))


def _worst_bits16(key_type: str, largest: bool) -> int:
    """The 16-bit word that ranks last in the requested order among the values a caller fills with: -inf / +inf for the float
    types (NaNs rank beyond them, but a filter fills with a number), the type's lowest / highest value for the integer ones."""
    lowest, highest = {"uint16": (0x0000, 0xFFFF), "int16": (0x8000, 0x7FFF), "float16": (0xFC00, 0x7C00),
                       "bfloat16": (0xFF80, 0x7F80)}[key_type]
    return lowest if largest else highest


def _fill_bits16(dtype, fill, largest: bool) -> int:
    """The 16-bit word ``topk16_filter_rows`` fills with: ``fill`` as a value of ``dtype`` (``None``: the worst value in the
    requested order)."""
    torch = _torch()
    if fill is None:
        return _worst_bits16(_dtype_name(dtype), largest)
    if dtype == torch.int16:
        if isinstance(fill, float) and not fill.is_integer():
            raise ValueError("fill: an integer for an int16 tensor")
        if not -(1 << 15) <= int(fill) < (1 << 15):
            raise ValueError("fill: within the range of int16")
        return int(fill) & 0xFFFF
    return int(torch.tensor(float(fill), dtype=dtype).view(torch.int16).item()) & 0xFFFF


def _k_per_row(k, rows: int, device):
    """``k`` of ``topk16_filter_rows`` as the int32 vector the library reads, one entry per row, on ``device``: an int (every row),
    a sequence of ints, or an int32 / int64 tensor.  Values outside int32 are clamped into it first -- both ends mean "filter off"
    (a negative entry reads as a uint32 above every row length).  An int32 tensor on ``device`` is used as it is."""
    torch = _torch()
    lo, hi = -(1 << 31), (1 << 31) - 1
    if isinstance(k, torch.Tensor):
        if k.dtype not in (torch.int32, torch.int64):
            raise TypeError("k: an int, a sequence of ints, or an int32 / int64 tensor")
        if k.numel() != rows:
            raise ValueError(f"k: one entry per row ({rows}), got {k.numel()}")
        if k.dtype == torch.int64:
            k = k.clamp(lo, hi).to(torch.int32)
        return k.to(device).contiguous().view(-1)
    if isinstance(k, (bool, str, bytes)):
        raise TypeError("k: an int, a sequence of ints, or an int32 / int64 tensor")
    if isinstance(k, int):
        return torch.full((rows,), min(max(k, lo), hi), dtype=torch.int32, device=device)
    try:
        values = [min(max(int(v), lo), hi) for v in k]
    except TypeError:
        raise TypeError("k: an int, a sequence of ints, or an int32 / int64 tensor") from None
    if len(values) != rows:
        raise ValueError(f"k: one entry per row ({rows}), got {len(values)}")
    return torch.tensor(values, dtype=torch.int32).to(device)


def GPUTopK16Filter(d_keys, d_k, key_type: str = "int16", largest: bool = True, fill: int | None = None, out=None, workspace=None,
                    stream=None, check_fault: bool = False):
    """The top-k filter of every row with a k of its own per row, read on the device (``lsdsort_topk16_filter_device``):
    ``d_keys`` as for ``GPUTopK16``, ``d_k`` a contiguous int32 CUDA tensor with one entry per row.  Row ``r`` of the result is row
    ``r`` of ``d_keys`` where ``d_k[r]`` (as uint32) is 0 or at least the row length -- the filter is off, -1 included.  Otherwise
    the keys at least as good as the ``d_k[r]``-th best of the row (``largest``: the largest) are kept bit for bit, every duplicate
    of that value included, and the others become the 16-bit word ``fill`` (an int in 0 .. 0xFFFF; ``None``: -inf / +inf for the
    float types, the type's lowest / highest value for the integer ones, by ``largest``).  The order is the library's total order:
    -0.0 below +0.0, NaNs by sign at the two ends.  Returns the result: ``out`` where one is given (``out=d_keys`` runs in place),
    else a new tensor.  The host never reads ``d_k``: a captured graph follows its contents.  Stream-ordered; short rows are read
    once and written once, rows above 16384 keys read three times and written once."""
    torch = _torch()
    code, rows, cols = _keys16(d_keys, key_type, "is filtered")
    _per_row(d_k, "d_k", rows, torch.int32)
    fill = _fill16(fill, key_type, bool(largest))
    _row_out(out, d_keys)
    with _on_stream(stream):   # the output, like a temporary workspace, belongs to the stream the kernels run on
        result = out if out is not None else torch.empty_like(d_keys)
    workspace = _workspace(workspace, "lsdsort_topk16_filter_workspace_bytes", (rows, cols), d_keys.device, stream)
    check(lib().lsdsort_topk16_filter_device(d_keys.data_ptr(), rows, cols, d_k.data_ptr(), code, int(bool(largest)), fill,
                                             result.data_ptr(), workspace.data_ptr(), workspace.numel(), _stream(stream)),
          "lsdsort_topk16_filter_device")
    if check_fault and rows and cols:
        _check_fault(workspace, stream)
    return result


def topk16_filter_rows(x, k, largest: bool = True, fill=None, inplace: bool = False, stream=None):
    """The top-k filter of a sampling step for a float16 / bfloat16 / int16 CUDA tensor of one or more dimensions: per row of the
    last dimension, ``thr = torch.topk(row, k_r, largest=largest).values[-1]`` and ``row.masked_fill(row < thr, fill)`` (``>`` for
    smallest), without the top-k, its gather and the mask: every key at least as good as the ``k_r``-th best stays, ties of it
    included.  ``k`` is an int for every row, or one entry per row as a sequence or an int32 / int64 tensor; ``k_r <= 0`` or
    ``k_r >= `` the row length leaves the row as it is.  A host value becomes a device tensor here; an int32 CUDA tensor is used as
    it is, so a captured caller pays no conversion and may change its contents between replays.  ``fill``: a value of ``x``'s dtype;
    ``None`` is -inf for ``largest`` and +inf for smallest, on int16 the lowest / highest value.  ``inplace`` filters ``x`` itself
    (contiguous) and returns it.  The order is the library's total order, not torch's: -0.0 ranks below +0.0 and NaNs sort by sign
    at the two ends."""
    torch = _torch()
    r = _Rows(x, (torch.int16, torch.float16, torch.bfloat16), contiguous=bool(inplace))
    rows = r.rows
    bits = _fill_bits16(x.dtype, fill, bool(largest))
    with _on_stream(stream):
        d_k = _k_per_row(k, rows, x.device)
        if rows == 0 or r.cols == 0:
            return x if inplace else x.clone()
        flat = r.flat(copy=not inplace)
        out = GPUTopK16Filter(flat, d_k, key_type=r.key_type, largest=largest, fill=bits, out=flat if inplace else None, stream=stream)
        return x if inplace else out.view(x.shape)


def topp16_filter_workspace_bytes(rows: int, cols: int) -> int:
    """Bytes of device workspace ``GPUTopP16Filter`` needs for ``rows`` rows of ``cols`` 16-bit keys (whatever the p's)."""
    return int(lib().lsdsort_topp16_filter_workspace_bytes(rows, cols))


def _p_per_row(p, rows: int, device, name: str = "p"):
    """A per-row float argument (``p`` of ``topp16_filter_rows``, ``u`` of ``sample16_rows``) as the float32 vector the library
    reads, one entry per row, on ``device``: a float (every row), a sequence of floats, or a float32 / float64 tensor.  A float32
    tensor on ``device`` is used as it is.  ``name``: what the messages call it."""
    torch = _torch()
    what = f"{name}: a float, a sequence of floats, or a float32 / float64 tensor"
    if isinstance(p, torch.Tensor):
        if p.dtype not in (torch.float32, torch.float64):
            raise TypeError(what)
        if p.numel() != rows:
            raise ValueError(f"{name}: one entry per row ({rows}), got {p.numel()}")
        return p.to(torch.float32).to(device).contiguous().view(-1)
    if isinstance(p, (bool, str, bytes)) or p is None:
        raise TypeError(what)
    if isinstance(p, (int, float)):
        return torch.full((rows,), float(p), dtype=torch.float32, device=device)
    try:
        values = [float(v) for v in p]
    except (TypeError, ValueError):
        raise TypeError(what) from None
    if len(values) != rows:
        raise ValueError(f"{name}: one entry per row ({rows}), got {len(values)}")
    return torch.tensor(values, dtype=torch.float32).to(device)


def GPUTopP16Filter(d_keys, d_p, key_type: str = "bfloat16", fill: int | None = None, out=None, workspace=None, stream=None,
                    check_fault: bool = False, d_min_p=None, d_temperature=None):
    """The top-p (nucleus) filter of every row with a p of its own per row, read on the device (``lsdsort_topp16_filter_device``):
    ``d_keys`` a contiguous 1-D or 2-D float16 / bfloat16 CUDA tensor of logits, ``d_p`` a contiguous float32 CUDA tensor with one
    entry per row.  Row ``r`` of the result is row ``r`` of ``d_keys`` where ``d_p[r]`` is not below 1 (a NaN included): the filter
    is off.  Otherwise the smallest set of the row's best keys whose softmax mass reaches ``d_p[r]`` is kept bit for bit -- a key
    stays iff the mass of the strictly better keys is below ``d_p[r]``, or it is the row's best value; every duplicate of a kept
    value stays -- and the others become the 16-bit word ``fill`` (an int in 0 .. 0xFFFF; ``None``: -inf).  The order is the
    library's total order: -0.0 below +0.0, NaNs by sign at the two ends, and a NaN has no mass.  The threshold is found without a
    sort, in float32 and 64-bit fixed point: it is consistent with ``d_p[r]`` to 2^-12 of the row's mass, and the result is the same
    bits on every call, whatever the other rows.  Returns the result: ``out`` where one is given (``out=d_keys`` runs in place),
    else a new tensor.  The host never reads ``d_p``: a captured graph follows its contents.  Stream-ordered; short rows are read
    once and written once, rows above 16384 keys read four times and written once.

    ``d_min_p`` and ``d_temperature`` (``lsdsort_topp16_filter_ex_device``; without them the entry above is called as before) are
    contiguous float32 CUDA tensors with one entry per row, read on the device like ``d_p``.  The masses become
    ``exp((x - m) / T_r)``; ``T_r`` not above 0 (a NaN included) is greedy: the maximum alone has mass.  With ``d_min_p`` a key also
    has to reach ``min_p_r`` times the best key's probability, ``value >= m + T_r ln(min_p_r)``; ``min_p_r`` not above 0 is off.  A
    key stays iff it passes both filters.  ``d_p`` may be ``None`` (top-p off in every row) when ``d_min_p`` is given."""
    torch = _torch()
    code, rows, cols = _logits16(d_keys, key_type, "is filtered")
    _per_row(d_p, "d_p", rows, torch.float32, optional=d_min_p is not None)
    _per_row(d_min_p, "d_min_p", rows, torch.float32, optional=True)
    _per_row(d_temperature, "d_temperature", rows, torch.float32, optional=True)
    fill = _fill16(fill, key_type, True)
    _row_out(out, d_keys)
    with _on_stream(stream):   # the output, like a temporary workspace, belongs to the stream the kernels run on
        result = out if out is not None else torch.empty_like(d_keys)
    workspace = _workspace(workspace, "lsdsort_topp16_filter_workspace_bytes", (rows, cols), d_keys.device, stream)
    if d_min_p is None and d_temperature is None:
        check(lib().lsdsort_topp16_filter_device(d_keys.data_ptr(), rows, cols, d_p.data_ptr(), code, fill, result.data_ptr(),
                                                 workspace.data_ptr(), workspace.numel(), _stream(stream)), "lsdsort_topp16_filter_device")
    else:
        check(lib().lsdsort_topp16_filter_ex_device(d_keys.data_ptr(), rows, cols, _ptr(d_p), _ptr(d_min_p), _ptr(d_temperature), code,
                                                    fill, result.data_ptr(), workspace.data_ptr(), workspace.numel(), _stream(stream)),
              "lsdsort_topp16_filter_ex_device")
    if check_fault and rows and cols:
        _check_fault(workspace, stream)
    return result


def topp16_filter_rows(x, p, fill=None, inplace: bool = False, stream=None, min_p=None, temperature=None):
    """The top-p (nucleus) filter of a sampling step for a float16 / bfloat16 CUDA tensor of logits of one or more dimensions: per
    row of the last dimension what sort descending, softmax, ``cumsum - probs >= p`` masked and scattered back gives, without the
    sort: the best logits stay until their softmax mass reaches ``p_r``, ties of a kept value included, and the others become
    ``fill``.  ``p`` is a float for every row, or one entry per row as a sequence or a float32 / float64 tensor; ``p_r >= 1`` or a
    NaN leaves the row as it is, ``p_r <= 0`` keeps the best value alone.  A host value becomes a device tensor here; a float32 CUDA
    tensor is used as it is, so a captured caller pays no conversion and may change its contents between replays.  ``fill``: a value
    of ``x``'s dtype; ``None`` is -inf.  ``inplace`` filters ``x`` itself (contiguous) and returns it.  The order is the library's
    total order, not torch's: -0.0 ranks below +0.0 and NaNs sort by sign at the two ends.  ``min_p`` and ``temperature`` take the
    forms of ``p``: with a temperature the softmax is that of ``x / T_r`` (``T_r <= 0``: greedy) without rounding ``x / T_r`` to 16
    bits, and with ``min_p`` a kept key also has at least ``min_p_r`` times the best key's probability (``min_p_r <= 0``: off); a
    row keeps what passes both.  ``p`` may be ``None`` (top-p off) when ``min_p`` is given."""
    torch = _torch()
    r = _Rows(x, (torch.float16, torch.bfloat16), contiguous=bool(inplace))
    rows = r.rows
    bits = _fill_bits16(x.dtype, fill, True)
    with _on_stream(stream):
        d_p = _p_per_row(p, rows, x.device) if p is not None or min_p is None else None
        d_min_p = _p_per_row(min_p, rows, x.device, "min_p") if min_p is not None else None
        d_t = _p_per_row(temperature, rows, x.device, "temperature") if temperature is not None else None
        if rows == 0 or r.cols == 0:
            return x if inplace else x.clone()
        flat = r.flat(copy=not inplace)
        out = GPUTopP16Filter(flat, d_p, key_type=r.key_type, fill=bits, out=flat if inplace else None, stream=stream,
                              d_min_p=d_min_p, d_temperature=d_t)
        return x if inplace else out.view(x.shape)


def sample16_workspace_bytes(rows: int, cols: int) -> int:
    """Bytes of device workspace ``GPUSample16`` needs for ``rows`` rows of ``cols`` 16-bit keys (whatever the u's, with or without
    logprobs)."""
    return int(lib().lsdsort_sample16_workspace_bytes(rows, cols))


def GPUSample16(d_keys, d_u, key_type: str = "bfloat16", out=None, logprobs=False, workspace=None, stream=None,
                check_fault: bool = False, d_temperature=None):
    """The draw of a sampling step, one token per row, with a uniform ``u`` of its own per row read on the device
    (``lsdsort_sample16_device``): ``d_keys`` a contiguous 1-D or 2-D float16 / bfloat16 CUDA tensor of logits, ``d_u`` a contiguous
    float32 CUDA tensor with one entry per row.  Row ``r`` of the result is the position ``i`` whose softmax mass interval, in position
    order, holds ``d_u[r]``: ``C_i <= u Z < C_i + w_i`` with the top-p filter's weights (0 for a NaN, 1 at the row's largest number,
    ``exp(x - m)`` elsewhere) -- what ``searchsorted(cumsum(softmax(row)), u, right=True)`` gives.  A key without mass (a NaN, a -inf
    under a finite maximum: what the filters fill with) is never drawn; ``u <= 0`` or a NaN draws the first key that has mass,
    ``u >= 1`` the last; a row that holds no number gives -1 (and a NaN logprob).  Integer fixed-point masses: the index is
    consistent with ``d_u[r]`` to 2^-12 of the row's mass and is the same on every call, whatever the other rows.  Returns the int32
    index tensor ``[rows]`` (``out`` where one is given); with ``logprobs`` -- ``True``, or a contiguous float32 CUDA tensor
    ``[rows]`` to fill -- ``(index, logprob)``, the drawn key's log-probability under the row's softmax in float32.  The host never
    reads ``d_u``: a captured graph follows its contents and the keys'.  Stream-ordered; ``d_keys`` is only read: rows of up to
    16384 keys once, longer ones twice plus one chunk.

    ``d_temperature`` (``lsdsort_sample16_ex_device``; without it the entry above is called as before): a contiguous float32 CUDA
    tensor with one entry per row, read on the device.  The weights become ``exp((x - m) / T_r)`` and the logprob is that of the
    tempered softmax; ``T_r`` not above 0 (a NaN included) is greedy: the argmax, uniform over its duplicates by ``u``."""
    torch = _torch()
    code, rows, cols = _logits16(d_keys, key_type, "is sampled")
    _per_row(d_u, "d_u", rows, torch.float32)
    _per_row(d_temperature, "d_temperature", rows, torch.float32, optional=True)
    _per_row(out, "out", rows, torch.int32, dims=(1,), optional=True)
    own_logprob = isinstance(logprobs, torch.Tensor)
    if own_logprob:
        _per_row(logprobs, "logprobs", rows, torch.float32, dims=(1,))
    elif not isinstance(logprobs, bool):
        raise TypeError("logprobs: a bool, or a contiguous 1-D float32 CUDA tensor")
    with _on_stream(stream):   # the outputs, like a temporary workspace, belong to the stream the kernels run on
        index = out if out is not None else torch.empty((rows,), dtype=torch.int32, device=d_keys.device)
        logprob = logprobs if own_logprob else (torch.empty((rows,), dtype=torch.float32, device=d_keys.device) if logprobs else None)
    workspace = _workspace(workspace, "lsdsort_sample16_workspace_bytes", (rows, cols), d_keys.device, stream)
    if d_temperature is None:
        check(lib().lsdsort_sample16_device(d_keys.data_ptr(), rows, cols, d_u.data_ptr(), code, index.data_ptr(), _ptr(logprob),
                                            workspace.data_ptr(), workspace.numel(), _stream(stream)), "lsdsort_sample16_device")
    else:
        check(lib().lsdsort_sample16_ex_device(d_keys.data_ptr(), rows, cols, d_u.data_ptr(), d_temperature.data_ptr(), code,
                                               index.data_ptr(), _ptr(logprob), workspace.data_ptr(), workspace.numel(), _stream(stream)),
              "lsdsort_sample16_ex_device")
    if check_fault and rows and cols:
        _check_fault(workspace, stream)
    return (index, logprob) if logprob is not None else index


def sample16_rows(x, u=None, top_k=None, top_p=None, generator=None, return_logprobs: bool = False, stream=None, min_p=None,
                  temperature=None):
    """One token per row of a float16 / bfloat16 CUDA tensor of logits of one or more dimensions, drawn from the softmax of the row of
    the last dimension: what ``torch.multinomial(torch.softmax(x.float(), -1), 1)`` draws, as the inverse CDF
    ``searchsorted(cumsum(softmax(row)), u_r, right=True)`` of a uniform ``u_r``, without the float32 passes.  ``u`` is a float for
    every row, or one entry per row as a sequence or a float32 / float64 tensor; a float32 CUDA tensor is used as it is, so a captured
    caller pays no conversion and changes its contents between replays; ``None`` draws ``torch.rand(rows, generator=generator)`` on
    ``x``'s device.  With ``top_k`` (the forms of ``topk16_filter_rows``) or ``top_p`` (those of ``topp16_filter_rows``) the filters
    run first, in place on ONE copy of ``x``, top-k before top-p, and the draw is over the renormalised survivors.  Returns int64
    indices of shape ``x.shape[:-1]``, with ``return_logprobs`` ``(indices, logprobs)``, the float32 log-probability of each drawn
    key (after the filters).  A row without a number gives -1.  A float32 ``u`` resolves 2^-24: a token whose probability is below
    that, late in a row, may be out of reach -- as with any float32 uniform.  ``temperature`` and ``min_p`` take the forms of
    ``top_p``: the softmax is that of ``x / T_r`` in the filters and in the draw (``T_r <= 0``: greedy, the argmax), and ``min_p``
    joins ``top_p`` in ONE filter call between top-k and the draw."""
    torch = _torch()
    r = _Rows(x, (torch.float16, torch.bfloat16))
    rows, cols, key_type = r.rows, r.cols, r.key_type
    with _on_stream(stream):
        if u is None:
            d_u = torch.rand((rows,), dtype=torch.float32, device=x.device, generator=generator)
        else:
            d_u = _p_per_row(u, rows, x.device, "u")
        d_k = _k_per_row(top_k, rows, x.device) if top_k is not None else None
        d_p = _p_per_row(top_p, rows, x.device, "top_p") if top_p is not None else None
        d_min_p = _p_per_row(min_p, rows, x.device, "min_p") if min_p is not None else None
        d_t = _p_per_row(temperature, rows, x.device, "temperature") if temperature is not None else None
        if rows == 0 or cols == 0:
            index = torch.full(x.shape[:-1], -1, dtype=torch.int64, device=x.device)
            logprob = torch.full(x.shape[:-1], float("nan"), dtype=torch.float32, device=x.device)
            return (index, logprob) if return_logprobs else index
        flat = r.flat()
        if d_k is not None or d_p is not None or d_min_p is not None:
            flat = flat.clone() if flat.data_ptr() == x.data_ptr() else flat   # the one copy the filters write
            if d_k is not None:
                GPUTopK16Filter(flat, d_k, key_type=key_type, largest=True, out=flat, stream=stream)
            if d_p is not None or d_min_p is not None:
                GPUTopP16Filter(flat, d_p, key_type=key_type, out=flat, stream=stream, d_min_p=d_min_p, d_temperature=d_t)
        got = GPUSample16(flat, d_u, key_type=key_type, logprobs=bool(return_logprobs), stream=stream, d_temperature=d_t)
        if return_logprobs:
            return r.restore(got[0].to(torch.int64)), r.restore(got[1])
        return r.restore(got.to(torch.int64))


def logprob16_workspace_bytes(rows: int, cols: int, slots: int) -> int:
    """Bytes of device workspace ``GPULogprob16`` needs for ``slots`` ids in each of ``rows`` rows of ``cols`` 16-bit keys (whatever the
    ids, with or without ranks and the log-sum-exp); 0 for a ``slots`` outside 1 .. ``LSDSORT_LOGPROB_MAX_SLOTS``."""
    return int(lib().lsdsort_logprob16_workspace_bytes(rows, cols, slots))


def _optional_out(arg, name: str, dtype, shape, device):
    """An optional output asked for as ``False`` (none), ``True`` (a new tensor) or a contiguous CUDA tensor of ``dtype`` with
    ``shape``'s element count to fill."""
    torch = _torch()
    if isinstance(arg, torch.Tensor):
        _dev(arg, name, (dtype,))
        if arg.numel() != int(np.prod(shape, dtype=np.int64)):
            raise ValueError(f"{name}: {int(np.prod(shape, dtype=np.int64))} entries, got {arg.numel()}")
        return arg
    if not isinstance(arg, bool):
        raise TypeError(f"{name}: a bool, or a contiguous {_dtype_name(dtype)} CUDA tensor")
    return torch.empty(shape, dtype=dtype, device=device) if arg else None


def GPULogprob16(d_keys, d_ids, key_type: str = "bfloat16", ranks=False, lse=False, d_temperature=None, out=None, workspace=None,
                 stream=None, check_fault: bool = False):
    """The log-probabilities of given tokens of every row (``lsdsort_logprob16_device``): ``d_keys`` a contiguous 1-D or 2-D float16 /
    bfloat16 CUDA tensor of logits, ``d_ids`` a contiguous int32 CUDA tensor ``[rows, slots]`` or ``[rows]`` (one slot), read on the
    device, with at most ``LSDSORT_LOGPROB_MAX_SLOTS`` slots.  Entry ``(r, s)`` of the result is the float32 log-probability of key
    ``d_ids[r, s]`` of row ``r`` under the row's softmax -- ``torch.log_softmax(row.float() / T_r, -1)[id]`` without the float32 row --
    from the masses and the integer sum of ``GPUSample16``: called on the index the draw returned it gives the bits of the draw's
    logprob.  A NaN key, an id below 0 or at or above the row length (padding) and a row without a number give NaN; a -inf under a
    finite maximum gives -inf.  ``ranks`` -- ``True``, or a contiguous int32 CUDA tensor of the ids' shape to fill -- adds the number of
    keys of the row that are numbers and strictly greater by value (``(row.float() > x).sum()``; -1 for a NaN key and for padding);
    ``lse`` -- ``True``, or a float32 CUDA tensor ``[rows]`` -- adds the log-sum-exp of the tempered row (NaN for a greedy row and a row
    without a number).  ``d_temperature``: a contiguous float32 CUDA tensor with one entry per row, as in ``GPUSample16`` (``T_r`` not
    above 0: greedy).  Returns the logprob tensor (``out`` where one is given), or with ``ranks`` / ``lse`` the tuple
    ``(logprob[, rank][, lse])``.  The host reads none of the arrays: a captured graph follows their contents.  Stream-ordered;
    ``d_keys`` is only read: rows of up to 16384 keys once, longer ones twice."""
    torch = _torch()
    code, rows, cols = _logits16(d_keys, key_type, "is scored")
    _dev(d_ids, "d_ids", (torch.int32,), dims=(1, 2))
    if d_ids.shape[0] != rows:
        raise ValueError(f"d_ids: one row of ids per row ({rows}), got {d_ids.shape[0]}")
    slots = 1 if d_ids.dim() == 1 else d_ids.shape[1]
    if not 1 <= slots <= errors.LSDSORT_LOGPROB_MAX_SLOTS:
        raise ValueError(f"d_ids: 1 .. {errors.LSDSORT_LOGPROB_MAX_SLOTS} ids per row, got {slots}")
    _per_row(d_temperature, "d_temperature", rows, torch.float32, optional=True)
    if out is not None:
        _dev(out, "out", (torch.float32,))
        if out.numel() != rows * slots:
            raise ValueError(f"out: one entry per id ({rows * slots}), got {out.numel()}")
    with _on_stream(stream):   # the outputs, like a temporary workspace, belong to the stream the kernels run on
        logprob = out if out is not None else torch.empty(d_ids.shape, dtype=torch.float32, device=d_keys.device)
        rank = _optional_out(ranks, "ranks", torch.int32, d_ids.shape, d_keys.device)
        total = _optional_out(lse, "lse", torch.float32, (rows,), d_keys.device)
    workspace = _workspace(workspace, "lsdsort_logprob16_workspace_bytes", (rows, cols, slots), d_keys.device, stream)
    check(lib().lsdsort_logprob16_device(d_keys.data_ptr(), rows, cols, d_ids.data_ptr(), slots, _ptr(d_temperature), code,
                                         logprob.data_ptr(), _ptr(rank), _ptr(total), workspace.data_ptr(), workspace.numel(),
                                         _stream(stream)), "lsdsort_logprob16_device")
    if check_fault and rows and cols:
        _check_fault(workspace, stream)
    got = (logprob,) + tuple(t for t in (rank, total) if t is not None)
    return got if len(got) > 1 else logprob


def logprobs16_rows(x, ids, temperature=None, return_ranks: bool = False, return_lse: bool = False, stream=None):
    """``torch.log_softmax(x.float() / T, -1).gather(-1, ids)`` for a float16 / bfloat16 CUDA tensor of logits of one or more
    dimensions, without the float32 passes over the rows: ``ids`` is an int32 / int64 CUDA tensor of shape ``x.shape[:-1]`` (one id per
    row: the sampled token, the next prompt token, a cross-entropy target) or ``x.shape[:-1] + (n,)``; the result has its shape.  An id
    below 0 or at or above the row length is padding and gives NaN, as does a NaN logit.  More than ``LSDSORT_LOGPROB_MAX_SLOTS`` ids
    per row take several calls.  ``temperature`` takes the forms of ``sample16_rows`` (``T_r <= 0``: greedy).  With ``return_ranks``
    also the int64 ranks ``(x.float() > x.gather(-1, ids)).sum(-1)`` (-1 for padding and NaN logits), with ``return_lse`` the float32
    log-sum-exp of every tempered row, of shape ``x.shape[:-1]``: ``(logprobs[, ranks][, lse])``."""
    torch = _torch()
    r = _Rows(x, (torch.float16, torch.bfloat16))
    _dev(ids, "ids", (torch.int32, torch.int64), contiguous=False)
    lead = r.lead
    if tuple(ids.shape) != lead and tuple(ids.shape[:-1]) != lead:
        raise ValueError(f"ids: the shape of x without its last dimension {lead}, or that with a last dimension of ids per row; got {tuple(ids.shape)}")
    rows, cols = r.rows, r.cols
    n = 1 if tuple(ids.shape) == lead else ids.shape[-1]
    step = errors.LSDSORT_LOGPROB_MAX_SLOTS
    with _on_stream(stream):
        d_t = _p_per_row(temperature, rows, x.device, "temperature") if temperature is not None else None
        if rows == 0 or cols == 0 or n == 0:
            got = (torch.full(ids.shape, float("nan"), dtype=torch.float32, device=x.device),)
            got += (torch.full(ids.shape, -1, dtype=torch.int64, device=x.device),) if return_ranks else ()
            got += (torch.full(lead, float("nan"), dtype=torch.float32, device=x.device),) if return_lse else ()
            return got if len(got) > 1 else got[0]
        flat = r.flat()
        wide = ids.reshape(rows, n)
        if wide.dtype != torch.int32:   # what does not fit 32 bits names no key
            wide = torch.where((wide < 0) | (wide >= cols), torch.full_like(wide, -1), wide).to(torch.int32)
        logprob = torch.empty((rows, n), dtype=torch.float32, device=x.device)
        rank = torch.empty((rows, n), dtype=torch.int32, device=x.device) if return_ranks else None
        total = None
        for a in range(0, n, step):
            part = wide[:, a:a + step].contiguous()
            got = GPULogprob16(flat, part, key_type=r.key_type, ranks=bool(return_ranks),
                               lse=bool(return_lse) and a == 0, d_temperature=d_t, stream=stream)
            got = got if isinstance(got, tuple) else (got,)
            logprob[:, a:a + step] = got[0]
            if return_ranks:
                rank[:, a:a + step] = got[1]
            if return_lse and a == 0:
                total = got[-1]
        out = (logprob.view(ids.shape),)
        out += (rank.view(ids.shape).to(torch.int64),) if return_ranks else ()
        out += (total.view(lead),) if return_lse else ()
        return out if len(out) > 1 else out[0]


def top_logprobs16_rows(x, n: int, temperature=None, stream=None):
    """The ``top_logprobs=n`` of a request in two calls and without a float32 row: ``topk16_rows(x, n)`` and the log-probabilities of
    its positions under the softmax of ``x / T`` -> ``(logprobs, indices)``, float32 and int64 of shape ``x.shape[:-1] + (n,)``, best
    first.  The order is ``topk16_rows``'s: +NaN logits come in front of +inf (their logprob is NaN), among equal logits the lower
    position first.  ``n`` may exceed ``LSDSORT_LOGPROB_MAX_SLOTS``."""
    torch = _torch()
    _dev(x, "x", (torch.float16, torch.bfloat16), contiguous=False)
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError("n: a positive int")
    _, indices = topk16_rows(x, n, largest=True, stream=stream)
    return logprobs16_rows(x, indices, temperature=temperature, stream=stream), indices


def rows16_workspace_bytes(rows: int, cols: int) -> int:
    """Bytes of device workspace ``GPUSortRows16`` needs for ``rows`` rows of ``cols`` 16-bit keys; the figure covers both routes."""
    return int(lib().lsdsort_rows16_workspace_bytes(rows, cols))


def set_rows16_route(route: int) -> None:
    """How ``GPUSortRows16`` sorts: -1 by row length (default), 0 always the widen route (map to uint32 with positions, the
    segmented sort, narrow), 1 the native kernels wherever they exist (rows of up to ``LSDSORT_ROWS16_NATIVE_MAX_COLS`` keys)."""
    check(lib().lsdsort_set_rows16_route(route), "lsdsort_set_rows16_route")


def GPUSortRows16(d_keys, key_type: str = "int16", descending: bool = False, return_indices: bool = True, out=None, workspace=None,
                  stream=None, check_fault: bool = False):
    """The stable sort of every row of ``d_keys`` (``lsdsort_rows16_device``): a contiguous 1-D (one row) or 2-D int16, float16 or
    bfloat16 CUDA tensor whose 16 bits compare as ``key_type``, paired with the dtype as in ``GPUSort16``: "uint16" / "int16" for an
    int16 tensor, "float16" / "bfloat16" for the tensor of that dtype (IEEE total order).  Returns ``(values, indices)``: ``values``
    in the input's shape and dtype (``out`` where one is given; ``out=d_keys`` sorts in place), ``indices`` the int32 positions
    within the row, or ``None`` without ``return_indices``.  Equal keys come out in position order in either direction.
    Stream-ordered; ``d_keys`` is only read unless it is ``out``."""
    torch = _torch()
    code, rows, cols = _keys16(d_keys, key_type, "sorts")
    _row_out(out, d_keys)
    with _on_stream(stream):   # the outputs, like a temporary workspace, belong to the stream the kernels run on
        values = out if out is not None else torch.empty_like(d_keys)
        indices = torch.empty(d_keys.shape, dtype=torch.int32, device=d_keys.device) if return_indices else None
    workspace = _workspace(workspace, "lsdsort_rows16_workspace_bytes", (rows, cols), d_keys.device, stream)
    check(lib().lsdsort_rows16_device(d_keys.data_ptr(), rows, cols, code, int(bool(descending)), values.data_ptr(), _ptr(indices),
                                      workspace.data_ptr(), workspace.numel(), _stream(stream)), "lsdsort_rows16_device")
    if check_fault and rows and cols:
        _check_fault(workspace, stream)
    return values, indices


def sort_rows16(x, descending: bool = False, return_indices: bool = False, stream=None):
    """``torch.sort(x, dim=-1, stable=True, descending=descending)`` for an int16 / float16 / bfloat16 CUDA tensor of one or more
    dimensions, the 16-bit counterpart of ``sort_rows``: returns the sorted copy, and with ``return_indices`` also the int64
    positions within each row (equal keys keep their input order in either direction).  The float types follow IEEE total order,
    not torch's: NaNs by sign at the two ends and -0.0 below +0.0."""
    torch = _torch()
    r = _Rows(x, (torch.int16, torch.float16, torch.bfloat16))
    with _on_stream(stream):
        values, indices = GPUSortRows16(r.flat(), key_type=r.key_type, descending=descending, return_indices=return_indices,
                                        stream=stream)
        if return_indices:
            return values.view(x.shape), indices.view(x.shape).to(torch.int64)
    return values.view(x.shape)


# ------------------------------------------------------------------------------ run-length encode and unique
def rle_workspace_bytes(n: int, key_bits: int = 32) -> int:
    """Bytes of device workspace ``GPURunLength`` needs for up to ``n`` keys of ``key_bits`` (32 | 64), whatever outputs are asked
    for; 0 above the limit or for another width."""
    return int(lib().lsdsort_rle_workspace_bytes(n, key_bits))


def unique_workspace_bytes(n: int, key_type: str = "int32", with_positions: bool = False) -> int:
    """Bytes of device workspace ``GPUUnique`` needs for up to ``n`` keys of ``key_type`` (any of the six 32- and 64-bit names);
    ``with_positions``: ``first`` or ``inverse`` is asked for.  0 above the limit."""
    return int(lib().lsdsort_unique_workspace_bytes(n, _key_type(key_type, {**KEY_TYPES_32, **KEY_TYPES_64}), int(bool(with_positions))))


def _word_keys(d_keys, name: str, key_type=None, contiguous: bool = True):
    """The key check of the run-length and unique wrappers: a 1-D CUDA tensor of 32- or 64-bit elements.  Returns the name of the
    key type its bits compare as: ``key_type`` where one is given -- of the tensor's width, and for a float tensor its own -- or
    the tensor's dtype."""
    torch = _torch()
    own = {torch.int32: "int32", torch.float32: "float32", torch.int64: "int64", torch.float64: "float64"}
    for unsigned in ("uint32", "uint64"):   # where torch has them
        if hasattr(torch, unsigned):
            own[getattr(torch, unsigned)] = unsigned
    _dev(d_keys, name, tuple(own), dims=(1,), contiguous=contiguous)
    if key_type is None:
        return own[d_keys.dtype]
    table = KEY_TYPES_32 if d_keys.element_size() == 4 else KEY_TYPES_64
    _key_type(key_type, {**KEY_TYPES_32, **KEY_TYPES_64})
    if key_type not in table or (d_keys.dtype.is_floating_point and key_type != own[d_keys.dtype]):
        fits = (own[d_keys.dtype],) if d_keys.dtype.is_floating_point else tuple(table)
        raise TypeError(f"a {own[d_keys.dtype]} tensor compares with key_type " + " or ".join(f'"{k}"' for k in fits))
    return key_type


_RUN_OUTS = (("out", "keys", "runs"), ("out_vals", "values", "aggregates"))   # what the messages call the outputs and their inputs


def _run_outputs(d_keys, outs, optional, may_alias: bool, stream):
    """The outputs of the four run units -> (mandatory ones, optional ones, num).  ``outs``: ``(out, input)`` for the keys, and
    for the reduces the values: ``out`` is ``None`` (a new tensor like the input) or a contiguous CUDA tensor of the input's dtype
    and length -- the input itself only where ``may_alias``.  ``optional``: ``(argument, name)`` of every int32 array of the keys'
    length that ``_optional_out`` makes, fills or leaves out.  ``num``: the one-word int32 count.  All under the stream: the
    outputs, like a temporary workspace, belong to the stream the kernels run on."""
    torch = _torch()
    for (out, src), (name, what, takes) in zip(outs, _RUN_OUTS):
        if out is None:
            continue
        _dev(out, name, (src.dtype,), dims=(1,))
        if out.numel() != src.numel():
            raise ValueError(f"{name}: as long as the {what} ({src.numel()}), got {out.numel()}")
        if not may_alias and out.numel() and out.data_ptr() == src.data_ptr():
            raise ValueError(f"{name}: the {what} themselves cannot take the {takes} (they are read while the runs are stored)")
    n = d_keys.numel()
    with _on_stream(stream):
        fixed = [out if out is not None else torch.empty_like(src) for out, src in outs]
        extra = [_optional_out(arg, name, torch.int32, (n,), d_keys.device) for arg, name in optional]
        num = torch.empty(1, dtype=torch.int32, device=d_keys.device)
    return fixed, extra, num


def _run_result(fixed, extra, num) -> tuple:
    """What the four run units return: the mandatory outputs, the optional ones that were asked for, the count."""
    return tuple(fixed) + tuple(t for t in extra if t is not None) + (num,)


def _slice_by_count(got) -> list:
    """``(full-length tensors ..., count)`` of a run unit -> the tensors cut to the count, which is read here: the one
    synchronisation of the slicing wrappers."""
    m = int(got[-1].item())
    return [t[:m] for t in got[:-1]]


def GPURunLength(d_keys, counts=False, starts=False, out=None, workspace=None, stream=None, check_fault: bool = False):
    """Run-length encode of ``d_keys`` as it lies, sorted or not (``lsdsort_rle_device``): the counterpart of
    ``torch.unique_consecutive(return_counts=True)`` on the device.  ``d_keys``: a contiguous 1-D CUDA tensor of 32- or 64-bit
    elements (int32, float32, int64, float64, and uint32 / uint64 where torch has them), only read.  Two keys are equal where their
    BITS are: -0.0 and +0.0 are two values, every NaN payload is one of its own.  Returns ``(keys[, counts][, starts], num_runs)``:
    FULL-LENGTH tensors whose first ``num_runs`` entries are the word, the length and the first position of every run (the rest is
    not written), and ``num_runs``, a one-word int32 CUDA tensor -- no host synchronisation; slice after reading it.  ``counts`` /
    ``starts``: ``True``, or a contiguous int32 CUDA tensor of the keys' length to fill; ``out``: where the keys go (not ``d_keys``)."""
    _word_keys(d_keys, "d_keys")
    n = d_keys.numel()
    bits = 8 * d_keys.element_size()
    fixed, extra, num = _run_outputs(d_keys, [(out, d_keys)], [(counts, "counts"), (starts, "starts")], False, stream)
    workspace = _workspace(workspace, "lsdsort_rle_workspace_bytes", (n, bits), d_keys.device, stream, "too many keys")
    check(lib().lsdsort_rle_device(_ptr(d_keys, n), n, bits, _ptr(fixed[0], n), _ptr(extra[0], n), _ptr(extra[1], n), num.data_ptr(),
                                   workspace.data_ptr(), workspace.numel(), _stream(stream)), "lsdsort_rle_device")
    if check_fault and n:
        _check_fault(workspace, stream)
    return _run_result(fixed, extra, num)


def GPUUnique(d_keys, key_type=None, descending: bool = False, counts=False, first=False, inverse=False, out=None, workspace=None,
              stream=None, check_fault: bool = False):
    """The distinct keys of ``d_keys`` in sorted order (``lsdsort_unique_device``): the library's sort on a copy inside the
    workspace, then the run-length kernels.  ``d_keys``: as for ``GPURunLength``; ``key_type``: how its bits compare -- by default
    as the tensor's dtype; an int32 / int64 tensor also as "uint32" / "float32" or "uint64" / "float64" (bit patterns) -- floats in
    IEEE total order; ``descending``: the largest first.  Equality is equality of bits, as in ``GPURunLength``: -0.0 and +0.0 are two
    values, every NaN payload is one of its own.  Returns
    ``(keys[, counts][, first][, inverse], num_unique)``: full-length tensors and the one-word int32 count, no host synchronisation.
    ``counts[j]``: how often value ``j`` occurs; ``first[j]``: the lowest input position that holds it; ``inverse[i]``: the ``j`` with
    ``keys[j] == d_keys[i]`` (all ``n`` entries written).  Each of the three: ``True``, or a contiguous int32 CUDA tensor of the keys'
    length to fill.  ``out``: where the distinct keys go; it may be ``d_keys`` itself."""
    key_type = _word_keys(d_keys, "d_keys", key_type)
    code = _key_type(key_type, {**KEY_TYPES_32, **KEY_TYPES_64})
    n = d_keys.numel()
    fixed, extra, num = _run_outputs(d_keys, [(out, d_keys)], [(counts, "counts"), (first, "first"), (inverse, "inverse")], True, stream)
    positions = extra[1] is not None or extra[2] is not None
    workspace = _workspace(workspace, "lsdsort_unique_workspace_bytes", (n, code, int(positions)), d_keys.device, stream, "too many keys")
    check(lib().lsdsort_unique_device(_ptr(d_keys, n), n, code, int(bool(descending)), _ptr(fixed[0], n), _ptr(extra[0], n),
                                      _ptr(extra[1], n), _ptr(extra[2], n), num.data_ptr(), workspace.data_ptr(), workspace.numel(),
                                      _stream(stream)), "lsdsort_unique_device")
    if check_fault and n:
        _check_fault(workspace, stream, "lsdsort_unique_check_device", n, code, int(positions))
    return _run_result(fixed, extra, num)


def unique(x, return_inverse: bool = False, return_counts: bool = False, return_index: bool = False, descending: bool = False):
    """``torch.unique(x, sorted=True, return_inverse=..., return_counts=...)`` for a 1-D int32 / float32 / int64 / float64 CUDA
    tensor (uint32 / uint64 where torch has them): returns the distinct values, then -- in this order, each where asked for -- the
    int64 ``inverse`` (``values[inverse] == x``), the int64 ``counts``, and with ``return_index`` (numpy's name) the int64 position
    of every value's first occurrence; ``descending``: the largest value first.  Reads the count once (one synchronisation) and
    slices.  Floats differ from torch where they must: the library compares BITS in IEEE total order, so -0.0 and +0.0 are two
    values (-0.0 first), every NaN payload is one value (torch keeps every NaN apart) and NaNs lie at the two ends by sign; the
    result equals torch's wherever the input holds no -0.0 next to a +0.0 and no NaN."""
    torch = _torch()
    _word_keys(x, "x", contiguous=False)
    got = list(GPUUnique(x.contiguous(), descending=descending, counts=bool(return_counts), first=bool(return_index),
                         inverse=bool(return_inverse)))
    inverse = [got.pop(-2)] if return_inverse else []   # all n entries: the one array that is not cut to the count
    values, *arrays = _slice_by_count(got)              # then counts and first, each where asked for
    result = (values,) + tuple(t.to(torch.int64) for t in inverse + arrays)
    return values if len(result) == 1 else result


def unique_consecutive(x, return_counts: bool = False):
    """``torch.unique_consecutive(x, return_counts=...)`` for a 1-D CUDA tensor of the types ``unique`` takes: the first element of
    every run of equal adjacent elements, and with ``return_counts`` the int64 run lengths.  One synchronisation (the count).
    Equality is equality of bits: the result equals torch's wherever the input holds no -0.0 next to a +0.0 and no NaN."""
    torch = _torch()
    _word_keys(x, "x", contiguous=False)
    values, *counts = _slice_by_count(GPURunLength(x.contiguous(), counts=bool(return_counts)))
    return (values, counts[0].to(torch.int64)) if return_counts else values


# ------------------------------------------------------------------------------ reduce by key
def reduce_runs_workspace_bytes(n: int, key_bits: int = 32) -> int:
    """Bytes of device workspace ``GPUReduceRuns`` needs for up to ``n`` keys of ``key_bits`` (32 | 64), whatever the values, the
    operation and the outputs; 0 above the limit or for another width."""
    return int(lib().lsdsort_reduce_runs_workspace_bytes(n, key_bits))


def reduce_by_key_workspace_bytes(n: int, key_type: str = "int32") -> int:
    """Bytes of device workspace ``GPUReduceByKey`` needs for up to ``n`` keys of ``key_type`` (any of the six 32- and 64-bit names);
    0 above the limit."""
    return int(lib().lsdsort_reduce_by_key_workspace_bytes(n, _key_type(key_type, {**KEY_TYPES_32, **KEY_TYPES_64})))


def _reduce_values(d_vals, n: int, op: str):
    """The value check of the reduce wrappers: a contiguous 1-D int32 / float32 CUDA tensor (uint32 where torch has it) as long as
    the keys, and one of the three operations.  Returns the header's codes ``(val_type, op)``; the value type follows the dtype."""
    torch = _torch()
    own = {torch.int32: "int32", torch.float32: "float32"}
    if hasattr(torch, "uint32"):
        own[torch.uint32] = "uint32"
    _dev(d_vals, "d_vals", tuple(own), dims=(1,))
    if d_vals.numel() != n:
        raise ValueError("keys and values differ in length")
    if op not in errors.REDUCE_OPS:
        raise ValueError("op: " + " or ".join(f'"{name}"' for name in errors.REDUCE_OPS) + f", got {op!r}")
    return errors.VAL_TYPES[own[d_vals.dtype]], errors.REDUCE_OPS[op]


def GPUReduceRuns(d_keys, d_vals, op: str = "sum", counts=False, out_keys=None, out_vals=None, workspace=None, stream=None,
                  check_fault: bool = False):
    """``op`` ("sum" | "min" | "max") of ``d_vals`` over every run of equal adjacent keys of ``d_keys`` as it lies, sorted or not
    (``lsdsort_reduce_runs_device``): ``torch.unique_consecutive`` plus a segment reduce, on the device and without atomics.
    ``d_keys``: as for ``GPURunLength`` (keys are equal where their BITS are); ``d_vals``: a contiguous 1-D int32 / float32 CUDA
    tensor (uint32 where torch has it) of the same length, whose dtype says how the values are read.  Integer sums wrap; float min /
    max follow the library's total order (-NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN) and return the bits of one of the run's
    values; float sums are IEEE additions in an order fixed by the positions, the same bits on every call, and a run of one element
    keeps its bits.  Returns ``(keys, aggregates[, counts], num_runs)``: FULL-LENGTH tensors whose first ``num_runs`` entries are
    written, and the one-word int32 count -- no host synchronisation.  ``counts``: ``True``, or a contiguous int32 CUDA tensor of the
    keys' length to fill; ``out_keys`` / ``out_vals``: where keys and aggregates go (not the inputs themselves)."""
    _word_keys(d_keys, "d_keys")
    n = d_keys.numel()
    bits = 8 * d_keys.element_size()
    val_type, code = _reduce_values(d_vals, n, op)
    fixed, extra, num = _run_outputs(d_keys, [(out_keys, d_keys), (out_vals, d_vals)], [(counts, "counts")], False, stream)
    workspace = _workspace(workspace, "lsdsort_reduce_runs_workspace_bytes", (n, bits), d_keys.device, stream, "too many keys")
    check(lib().lsdsort_reduce_runs_device(_ptr(d_keys, n), _ptr(d_vals, n), n, bits, val_type, code, _ptr(fixed[0], n), _ptr(fixed[1], n),
                                           _ptr(extra[0], n), num.data_ptr(), workspace.data_ptr(), workspace.numel(), _stream(stream)),
          "lsdsort_reduce_runs_device")
    if check_fault and n:
        _check_fault(workspace, stream)
    return _run_result(fixed, extra, num)


def GPUReduceByKey(d_keys, d_vals, op: str = "sum", key_type=None, descending: bool = False, counts=False, out_keys=None, out_vals=None,
                   workspace=None, stream=None, check_fault: bool = False):
    """``op`` of ``d_vals`` per DISTINCT key of the unsorted ``d_keys``, the keys in sorted order (``lsdsort_reduce_by_key_device``):
    the library's stable pair sort on copies inside the workspace, then the kernels of ``GPUReduceRuns`` -- what
    ``index_add_`` / ``scatter_reduce_`` on ``unique``'s inverse map do with atomics, here in a fixed order: the values of a group
    meet in input order and the same input gives the same bits on every call.  ``key_type`` and ``descending``: as for ``GPUUnique``;
    values, operations and their float rules (-0.0, NaN, the total order of min / max): as for ``GPUReduceRuns``.  Returns
    ``(keys, aggregates[, counts], num_groups)``: full-length tensors and the one-word int32 count, no host synchronisation.
    ``out_keys`` / ``out_vals`` may be ``d_keys`` / ``d_vals`` themselves."""
    key_type = _word_keys(d_keys, "d_keys", key_type)
    key_code = _key_type(key_type, {**KEY_TYPES_32, **KEY_TYPES_64})
    n = d_keys.numel()
    val_type, code = _reduce_values(d_vals, n, op)
    fixed, extra, num = _run_outputs(d_keys, [(out_keys, d_keys), (out_vals, d_vals)], [(counts, "counts")], True, stream)
    workspace = _workspace(workspace, "lsdsort_reduce_by_key_workspace_bytes", (n, key_code), d_keys.device, stream, "too many keys")
    check(lib().lsdsort_reduce_by_key_device(_ptr(d_keys, n), _ptr(d_vals, n), n, key_code, int(bool(descending)), val_type, code,
                                             _ptr(fixed[0], n), _ptr(fixed[1], n), _ptr(extra[0], n), num.data_ptr(),
                                             workspace.data_ptr(), workspace.numel(), _stream(stream)), "lsdsort_reduce_by_key_device")
    if check_fault and n:
        _check_fault(workspace, stream, "lsdsort_reduce_by_key_check_device", n, key_code)
    return _run_result(fixed, extra, num)


def _reduce_sliced(reduce, keys, values, op: str, return_counts: bool):
    """The body of the two slicing wrappers; ``reduce(keys, values, counts)``: ``GPUReduceByKey`` or ``GPUReduceRuns``.  Strided
    1-D CUDA tensors are copied; any other ``values`` go to the shared check as they are."""
    torch = _torch()
    _word_keys(keys, "keys", contiguous=False)
    if isinstance(values, torch.Tensor) and values.is_cuda and values.dim() == 1 and not values.is_contiguous():
        values = values.contiguous()
    _reduce_values(values, keys.numel(), op)
    got = _slice_by_count(reduce(keys.contiguous(), values, bool(return_counts)))
    return tuple(got[:2]) + ((got[2].to(torch.int64),) if return_counts else ())


def reduce_by_key(keys, values, op: str = "sum", descending: bool = False, return_counts: bool = False):
    """``(distinct keys, op of the values that carry each[, counts])`` for 1-D CUDA tensors of equal length: ``keys`` of the types
    ``unique`` takes, ``values`` int32 / float32 (uint32 where torch has it), reinterpreted, never converted; ``op``: "sum", "min" or
    "max".  Equals ``torch.unique(return_inverse=True)`` followed by ``index_add_`` / ``scatter_reduce_(include_self=False)`` on
    integers and on NaN-free floats whose sums are exact; float sums are deterministic (``GPUReduceByKey``) and differ from a
    sequential sum by rounding.  -0.0 and +0.0 are two keys, every NaN payload is one.  Reads the count once (one synchronisation)
    and slices; ``return_counts`` adds the int64 group sizes."""
    return _reduce_sliced(lambda k, v, counts: GPUReduceByKey(k, v, op=op, descending=descending, counts=counts), keys, values, op,
                          return_counts)


def reduce_consecutive(keys, values, op: str = "sum", return_counts: bool = False):
    """``(the first key of every run of equal adjacent keys, op of the run's values[, counts])``: ``torch.unique_consecutive`` plus a
    segment reduce, for the tensors ``reduce_by_key`` takes.  One synchronisation (the count).  Keys are equal where their bits are:
    -0.0 and +0.0 end a run, NaN payloads that agree do not."""
    return _reduce_sliced(lambda k, v, counts: GPUReduceRuns(k, v, op=op, counts=counts), keys, values, op, return_counts)


def GPULSDRadixSortTimed(d_keys, r: int = 8, d_vals=None, algorithm: int = LSDSORT_ALGO_ONESWEEP, workspace=None,
                         stream=None) -> dict:
    """Same sort with per-kernel hipEvent times (``lsdsort_u32_device_timed``).  Blocking."""
    _dev(d_keys, "d_keys")
    n = d_keys.numel()
    pairs = d_vals is not None
    if pairs:
        _payload(d_vals, n)
    if workspace is None:
        workspace = alloc_workspace(n, r, pairs, algorithm, d_keys.device, stream)
    t = LsdsortTiming()
    st = lib().lsdsort_u32_device_timed(d_keys.data_ptr(), d_vals.data_ptr() if pairs else None, workspace.data_ptr(),
                                        workspace.numel(), n, r, algorithm, _stream(stream), ctypes.byref(t))
    check(st, "lsdsort_u32_device_timed")
    return {
        "total_ms": t.total_ms, "clear_ms": t.clear_ms, "histogram_ms": t.histogram_ms, "scan_ms": t.scan_ms,
        "scatter_ms": [t.scatter_ms[i] for i in range(t.passes)], "passes": t.passes, "tile_keys": t.tile_keys,
        "tiles": t.tiles, "hybrid": t.hybrid, "local_ms": t.local_ms,
    }


# ------------------------------------------------------------------------------ stage entries
def BuildHistograms(d_keys, r: int, bit_group: int, stream=None):
    """h[tile][digit] for one digit: ``BuildHistogramsKernel`` (.cu:660-702)."""
    torch = _torch()
    _dev(d_keys, "d_keys")
    n = d_keys.numel()
    tk = tile_keys(r)
    tiles = (n + tk - 1) // tk
    h = torch.empty((tiles, 1 << r), dtype=torch.int32, device=d_keys.device)
    check(lib().lsdsort_tile_histograms_u32_device(d_keys.data_ptr(), n, r, bit_group, h.data_ptr(), _stream(stream)),
          "lsdsort_tile_histograms_u32_device")
    return h


def BuildOffsets(d_hist, r: int, stream=None):
    """(local, global) offset tables from h[tile][digit]: the reference's .cu:862-895."""
    torch = _torch()
    _dev(d_hist, "d_hist")
    tiles = d_hist.shape[0]
    local = torch.empty_like(d_hist)
    glob = torch.empty_like(d_hist)
    scratch = _workspace(None, "lsdsort_tile_offsets_scratch_bytes", (tiles, r), d_hist.device, None, zero_ok=True)   # with the outputs
    check(lib().lsdsort_tile_offsets_u32_device(d_hist.data_ptr(), local.data_ptr(), glob.data_ptr(), tiles, r,
                                                scratch.data_ptr(), _stream(stream)),
          "lsdsort_tile_offsets_u32_device")
    return local, glob


def RankScatter(d_in, d_global, r: int, bit_group: int, d_vals=None, stream=None):
    """One rank-and-scatter pass from a global offset table: ``LSDRadixSortKernel`` (.cu:795-837)."""
    torch = _torch()
    _dev(d_in, "d_in")
    _dev(d_global, "d_global")
    out = torch.empty_like(d_in)
    vout = torch.empty_like(d_vals) if d_vals is not None else None
    check(lib().lsdsort_rank_scatter_u32_device(d_in.data_ptr(), out.data_ptr(),
                                                d_vals.data_ptr() if d_vals is not None else None,
                                                vout.data_ptr() if vout is not None else None, d_global.data_ptr(),
                                                d_in.numel(), r, bit_group, _stream(stream)),
          "lsdsort_rank_scatter_u32_device")
    return out if d_vals is None else (out, vout)


def DigitHistograms(d_keys, r: int, stream=None):
    """All 32/r digit histograms in one read (stage 1 of the default pass structure)."""
    torch = _torch()
    _dev(d_keys, "d_keys")
    h = torch.empty((32 // r, 1 << r), dtype=torch.int32, device=d_keys.device)
    check(lib().lsdsort_digit_histograms_u32_device(d_keys.data_ptr(), d_keys.numel(), r, h.data_ptr(),
                                                    _stream(stream)), "lsdsort_digit_histograms_u32_device")
    return h


def _partition(entry: str, d_keys, bits: int, stream, *cuts):
    """The body of the three partition faces: ``entry`` cuts ``d_keys`` into ``1 << bits`` buckets (``cuts``: its array of
    bounds, for the two that take one) -> (partitioned keys, int64 bucket counts).  Outputs and workspace are allocated on
    torch's current stream; the fault check synchronises ``stream`` before they are handed back."""
    torch = _torch()
    n = d_keys.numel()
    out = torch.empty_like(d_keys)
    counts = torch.zeros(1 << bits, dtype=torch.int64, device=d_keys.device)
    ws = _workspace(None, "lsdsort_msb_partition_workspace_bytes", (n, bits), d_keys.device, None, zero_ok=True)
    check(getattr(lib(), entry)(d_keys.data_ptr(), out.data_ptr(), n, bits, *cuts, counts.data_ptr(), ws.data_ptr(), ws.numel(),
                                _stream(stream)), entry)
    if n:
        _check_fault(ws, stream)
    return out, counts


def _cuts(values, what: str, ctype):
    """(bits, ctypes array) of a partition's 0, 1, 3 or 7 ascending bounds."""
    if len(values) not in (0, 1, 3, 7):
        raise ValueError(f"{what} count must be 0, 1, 3 or 7 (2, 4 or 8 buckets)")
    return (len(values) + 1).bit_length() - 1, (ctype * max(len(values), 1))(*values)


def MSBPartition(d_keys, msb_bits: int, stream=None):
    """Stable partition by the top ``msb_bits`` bits -> (partitioned keys, int64 bucket counts)."""
    _dev(d_keys, "d_keys")
    return _partition("lsdsort_msb_partition_u32_device", d_keys, msb_bits, stream)


def ThresholdPartition(d_keys, thresholds, stream=None):
    """Stable partition by 64-bit thresholds (1, 3 or 7 ascending values in [0, 2^32]; 2^32 = above every key):
    bucket(key) = number of thresholds <= key -> (partitioned keys, int64 bucket counts).  The form the sharded step's
    splitter rule uses (``lsdsort_threshold_partition_u32_device``)."""
    _dev(d_keys, "d_keys")
    bits, arr = _cuts([int(x) for x in thresholds], "threshold", ctypes.c_uint64)
    return _partition("lsdsort_threshold_partition_u32_device", d_keys, bits, stream, arr)


def SplitterPartition(d_keys, splitters, stream=None):
    """Stable partition by value: bucket(key) = number of ``splitters`` (ascending uint32 values, 1, 3 or 7 of
    them) <= key -> (partitioned keys, int64 bucket counts).  No splitters: one bucket."""
    _dev(d_keys, "d_keys")
    bits, arr = _cuts([int(x) & 0xFFFFFFFF for x in splitters], "splitter", ctypes.c_uint32)
    return _partition("lsdsort_splitter_partition_u32_device", d_keys, bits, stream, arr)


def sharded_thresholds(gathered, world: int, samples_per_rank: int, rank: int):
    """Host arithmetic of the sharded step's splitter rule (``lsdsort_sharded_thresholds``; no GPU): ``gathered`` is a
    [world][1 + samples_per_rank] uint32 array (valid count, then samples, per source rank) -> world - 1 thresholds
    of rank ``rank`` (Python ints in [0, 2^32])."""
    g = np.ascontiguousarray(gathered, dtype=np.uint32).reshape(world, 1 + samples_per_rank)
    out = (ctypes.c_uint64 * max(world - 1, 1))()
    check(lib().lsdsort_sharded_thresholds(g.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), world, samples_per_rank, rank, out),
          "lsdsort_sharded_thresholds")
    return [int(out[i]) for i in range(world - 1)]
