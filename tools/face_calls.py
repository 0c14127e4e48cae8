#!/usr/bin/env python3
"""Does the Python face of two trees make the same library calls?   tools/face_calls.py [--tree DIR] [--out FILE] [--time [--no-launch]]

What tools/isa_diff.py is to a kernel refactor, for lsdradixsort_amd/api.py.  Needs a GPU for its tensors and launches nothing:
``lsd.api.lib`` is replaced by a recorder that forwards the host-only size entries (``*_bytes``, ``lsdsort_tile_keys``) to the real
library, records every other entry's name and arguments and answers LSDSORT_OK.  Every ``GPU*`` wrapper, every torch-shaped
wrapper that reads no device result back, the stage entries and the partitions are called over the shapes and options that
reach every branch of the Python layer (``cases``), one line each: the call | the library calls | what came back; a case that
raises is recorded with the exception's type and text.  Pointers are named by the tensor they belong to, so that two runs
compare: the name of an argument of the call; ``r<i>``, the i-th tensor the wrapper returned, spelled out behind ``->`` as
``r0:i32[3,5]@0``; ``new:u8[3840]@0``, a tensor the wrapper made on the way (here a temporary workspace), each with dtype, shape
and the stream that was current when it was allocated (``@0`` torch's default stream, ``@side`` the case's own); ``NULL``.  Only
public names are used: the same file runs on any commit (``--tree``: the checkout whose package is
imported; default: this one).  Run it on two trees and ``diff`` the outputs: one differing line is a change of behaviour.

``--time`` instead measures the host time of three wrappers with a caller's workspace on the real library: wall time per call
over 2000 calls after a warm-up and a synchronise, ``GPUKth16`` on [8, 1024] bfloat16, ``GPUTopK`` on [8, 1024] int32 and
``GPUUnique`` on 1024 int32.  The device sets that pace wherever its kernels take longer than the wrapper; ``--time --no-launch``
times the same calls behind the recorder: the Python layer alone."""
import argparse
import ctypes
import os
import sys
import time

SIDE = None        # the case's own stream, where it has one
DEVICE = "cuda"


def tensor(dtype, *shape):
    import torch

    return torch.zeros(shape, dtype=dtype, device=DEVICE)


class Recorder:
    """stands in for the library"""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if name.endswith("_bytes") or "_bytes_" in name or name == "lsdsort_tile_keys":
            return getattr(self.real, name)

        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


def tracker():
    """A dispatch mode that remembers, per data pointer, the stream that was current when a tensor was first seen there."""
    import torch
    from torch.utils._python_dispatch import TorchDispatchMode

    class Tracker(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.seen = {}

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            out = func(*args, **(kwargs or {}))
            for t in (out if isinstance(out, (tuple, list)) else (out,)):
                if isinstance(t, torch.Tensor) and t.numel():
                    self.seen.setdefault(t.data_ptr(), (stream_label(current_stream()), t))
            return out
    return Tracker()


def current_stream():
    import torch

    return int(torch.cuda.current_stream().cuda_stream) if torch.cuda.is_available() else 0


def stream_label(handle):
    return "0" if not handle else ("side" if SIDE is not None and handle == int(SIDE.cuda_stream) else "other")


SHORT = {"int16": "i16", "int32": "i32", "int64": "i64", "uint8": "u8", "float16": "f16", "bfloat16": "bf16", "float32": "f32", "float64": "f64"}


def describe(t):
    return SHORT[str(t.dtype).replace("torch.", "")] + "[" + ",".join(map(str, t.shape)) + "]"


def tensors_of(value, prefix):
    """[(name, tensor)] of the tensors in an argument or a result, lists and tuples opened"""
    import torch

    if isinstance(value, torch.Tensor):
        return [(prefix, value)]
    if isinstance(value, (list, tuple)):
        return [pair for i, v in enumerate(value) for pair in tensors_of(v, f"{prefix}[{i}]")]
    return []


def render_result(value, names):
    import torch

    if isinstance(value, torch.Tensor):
        return names.get(id(value), "?")
    if isinstance(value, (list, tuple)):
        return "(" + ", ".join(render_result(v, names) for v in value) + ")"
    if isinstance(value, dict):
        return "{" + ", ".join(f"{k}: {render_result(v, names)}" for k, v in value.items()) + "}"
    return repr(value)


def run_case(lsd, label, name, kwargs):
    """the line of one case: the wrapper and its arguments | the library calls | what came back"""
    import torch

    rec = Recorder(REAL)
    lsd.api.lib = lambda: rec
    args = [pair for key, value in kwargs.items() for pair in tensors_of(value, key)]
    by_ptr = {}
    for key, t in args:
        if t.numel():
            by_ptr.setdefault(t.data_ptr(), key)
    track = tracker()
    try:
        with track:
            got = getattr(lsd, name)(**kwargs)
        raised = None
    except Exception as e:   # noqa: BLE001  (the exception IS the record)
        got, raised = None, f"{type(e).__name__}: {e}"
    returned, names = tensors_of(got, "r"), {}
    if isinstance(got, torch.Tensor):
        returned = [("r0", got)]
    for i, (_, t) in enumerate(returned):
        same = [key for key, a in args if a is t or (a.numel() and a.data_ptr() == t.data_ptr() and a.shape == t.shape and a.dtype == t.dtype)]
        where = track.seen.get(t.data_ptr(), ("?", None))[0] if t.numel() else "-"
        names[id(t)] = same[0] if same else f"r{i}:{describe(t)}@{where}"
        if t.numel() and not same:
            by_ptr.setdefault(t.data_ptr(), f"r{i}")

    def render(a):
        if a is None:
            return "NULL"
        if isinstance(a, ctypes.Array):
            return "[" + ",".join(render(v) for v in a) + "]"
        if isinstance(a, bool) or not isinstance(a, int):
            return "byref" if type(a).__name__ == "CArgObject" else repr(a)
        if a in by_ptr:
            return by_ptr[a]
        if a in track.seen:
            where, t = track.seen[a]
            return f"new:{describe(t)}@{where}"
        if SIDE is not None and a == int(SIDE.cuda_stream):
            return "side"
        return str(a) if a <= (1 << 32) else "pointer?"   # a size, a count, a threshold (2^32: above every key); else nobody's pointer

    def shown(key, value):
        made = tensors_of(value, key)
        return f"{key}=" + ("side" if key == "stream" else ",".join(describe(t) for _, t in made) if made else repr(value))

    calls = "; ".join(f"{entry.replace('lsdsort_', '')}(" + ", ".join(render(a) for a in a_) + ")" for entry, a_ in rec.calls)
    end = f"raises {raised}" if raised else f"-> {render_result(got, names)}"
    return [f"{name}({', '.join(shown(k, v) for k, v in kwargs.items())}) | {calls} | {end}"]


def cases():
    """(label, wrapper name, kwargs) of every case: per wrapper the base call on every shape it takes -- 1-D (8 keys), 2-D ([3, 40])
    where 2-D is taken, no rows, no columns -- and on the first of them the base call with one option changed, every option in turn:
    without indices, optional outputs as ``True`` and as a tensor, ``out=`` given and in place, a caller's workspace, ``check_fault``,
    a stream of the case's own, the ``_ex`` arguments.  Tensors are made when the case is: every case has fresh ones."""
    import torch

    i16, i32, i64, u8 = torch.int16, torch.int32, torch.int64, torch.uint8
    f16, bf16, f32, f64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
    common = {"workspace": lambda: tensor(u8, 1 << 20), "check_fault": True, "stream": lambda: SIDE}
    side = {"stream": lambda: SIDE}
    rows_of = lambda s: 1 if len(s) == 1 else s[0]   # noqa: E731
    per_row = lambda s, dtype=f32: (lambda: tensor(dtype, rows_of(s)))   # noqa: E731
    flat, rowed, nd = [(8,), (0,)], [(3, 40), (8,), (0, 40), (3, 0)], [(2, 3, 40), (8,), (0, 40), (3, 0)]
    out = []

    def add(name, shapes, build):
        for at, s in enumerate(shapes):
            base, options = build(s)
            out.append(("base", name, base))
            for key, value in (options.items() if at == 0 else ()):
                for v in (value if isinstance(value, list) else [value]):
                    out.append((key, name, dict(base, **{key: v() if callable(v) else v})))

    # ---- the 32-bit and wide sorts
    add("GPULSDRadixSort", flat, lambda s: (dict(d_keys=tensor(i32, *s)), dict(common, d_vals=lambda: tensor(i32, *s))))
    add("GPULSDRadixSortTimed", flat, lambda s: (dict(d_keys=tensor(i32, *s)), dict(d_vals=lambda: tensor(i32, *s), workspace=common["workspace"])))
    add("GPUSortMulti", flat, lambda s: (dict(d_keys=tensor(i32, *s), payloads=[tensor(i32, *s)]), dict(common, payloads=lambda: [tensor(i32, *s) for _ in range(3)])))
    add("GPUSortTyped", flat, lambda s: (dict(d_keys=tensor(f32, *s), key_type="float32"), dict(common, d_vals=lambda: tensor(i32, *s), descending=True)))
    add("GPUSortSegmented", flat, lambda s: (dict(d_keys=tensor(i32, *s), d_offsets=tensor(i32, 3)),
                                             dict(common, d_vals=lambda: tensor(i32, *s), d_offsets=[lambda: tensor(i32, 0), lambda: tensor(i32, 1)])))
    add("sort_rows", [(3, 40), (0, 40), (3, 0)], lambda s: (dict(x=tensor(f32, *s)), dict(side, return_indices=True)))
    add("GPUSortWide", flat, lambda s: (dict(d_keys=tensor(i64, *s)), dict(common, d_vals=[lambda: tensor(i32, *s), lambda: tensor(i64, *s)], key_type="int64")))
    add("GPUSortWide", [(8,)], lambda s: (dict(d_keys=tensor(i32, *s), d_vals=tensor(i64, *s)), dict(common)))
    add("sort64", flat, lambda s: (dict(x=tensor(i64, *s)), dict(side, return_indices=True, x=lambda: tensor(f64, 2 * s[0])[::2])))
    # ---- the row selects, 32-bit and 16-bit
    for bits, kind, tag in ((32, i32, "int32"), (16, bf16, "bfloat16")):
        sfx = "" if bits == 32 else "16"
        select = dict(common, return_indices=False, largest=True)
        add(f"GPUTopK{sfx}", rowed, lambda s: (dict(d_keys=tensor(kind, *s), k=min(5, s[-1]), key_type=tag), select))
        add(f"GPUKth{sfx}", rowed, lambda s: (dict(d_keys=tensor(kind, *s), rank=min(5, s[-1]), key_type=tag), select))
        add(f"GPUKth{sfx}Multi", rowed, lambda s: (dict(d_keys=tensor(kind, *s), ranks=[min(5, s[-1]), 0], key_type=tag), select))
        add(f"topk{sfx}_rows", nd, lambda s: (dict(x=tensor(kind, *s), k=min(5, s[-1])), dict(side, x=lambda: tensor(kind, *s[:-1], 2 * s[-1])[..., ::2])))
        add(f"kthvalue{sfx}_rows", nd, lambda s: (dict(x=tensor(kind, *s), k=min(5, s[-1])), side))
        add(f"median{sfx}_rows", nd, lambda s: (dict(x=tensor(kind, *s)), side))
        qkind = f32 if bits == 32 else bf16
        add(f"quantile{sfx}_rows", nd, lambda s: (dict(x=tensor(qkind, *s), q=0.5), dict(side, q=lambda: [0.1, 0.5, 0.9], interpolation="lower")))
    add("GPUTopK", [(3, 40)], lambda s: (dict(d_keys=tensor(f32, *s), k=5), {}))   # a float32 tensor as uint32: taken here, refused by the next two
    add("GPUKth", [(3, 40)], lambda s: (dict(d_keys=tensor(f32, *s), rank=5), {}))
    add("GPUKthMulti", [(3, 40)], lambda s: (dict(d_keys=tensor(f32, *s), ranks=[5]), {}))
    add("GPUKth16PerRow", rowed, lambda s: (dict(d_keys=tensor(bf16, *s), d_ranks=tensor(i32, rows_of(s)), key_type="bfloat16"),
                                            dict(common, return_indices=False, largest=True)))
    # ---- the 16-bit sorts
    add("GPUSort16", flat, lambda s: (dict(d_keys=tensor(i16, *s)), dict(common, d_vals=lambda: tensor(i32, *s), key_type="uint16")))
    add("sort16", flat, lambda s: (dict(x=tensor(bf16, *s)), dict(side, return_indices=True, x=lambda: tensor(i16, 2 * s[0])[::2])))
    add("GPUSortRows16", rowed, lambda s: (dict(d_keys=tensor(i16, *s)), dict(common, return_indices=False, out=lambda: tensor(i16, *s))))
    add("sort_rows16", nd, lambda s: (dict(x=tensor(bf16, *s)), dict(side, return_indices=True, x=lambda: tensor(i16, *s[:-1], 2 * s[-1])[..., ::2])))
    # ---- the filters, the draw, the log-probabilities
    add("GPUTopK16Filter", rowed, lambda s: (dict(d_keys=tensor(bf16, *s), d_k=tensor(i32, rows_of(s)), key_type="bfloat16"),
                                             dict(common, largest=False, fill=0x1234, out=lambda: tensor(bf16, *s))))
    add("GPUTopP16Filter", rowed, lambda s: (dict(d_keys=tensor(bf16, *s), d_p=tensor(f32, rows_of(s))),
                                             dict(common, fill=0x1234, out=lambda: tensor(bf16, *s), d_min_p=per_row(s), d_temperature=per_row(s))))
    add("GPUTopP16Filter", [(3, 40)], lambda s: (dict(d_keys=tensor(f16, *s), d_p=None, d_min_p=tensor(f32, 3), key_type="float16"), dict(d_temperature=per_row(s))))
    add("GPUSample16", rowed, lambda s: (dict(d_keys=tensor(bf16, *s), d_u=tensor(f32, rows_of(s))),
                                         dict(common, logprobs=[True, per_row(s)], out=per_row(s, i32), d_temperature=per_row(s))))
    add("GPULogprob16", rowed, lambda s: (dict(d_keys=tensor(bf16, *s), d_ids=tensor(i32, rows_of(s), 2)),
                                          dict(common, ranks=[True, lambda: tensor(i32, rows_of(s), 2)], lse=[True, per_row(s)], d_temperature=per_row(s),
                                               out=lambda: tensor(f32, rows_of(s), 2), d_ids=per_row(s, i32))))
    add("topk16_filter_rows", nd, lambda s: (dict(x=tensor(bf16, *s), k=5), dict(side, inplace=True, fill=0.5, k=lambda: tensor(i32, *s[:-1]))))
    add("topp16_filter_rows", nd, lambda s: (dict(x=tensor(bf16, *s), p=0.9), dict(side, inplace=True, min_p=0.1, temperature=0.7, p=lambda: tensor(f32, *s[:-1]))))
    add("sample16_rows", nd, lambda s: (dict(x=tensor(bf16, *s), u=0.5), dict(side, top_k=5, top_p=0.9, min_p=0.1, temperature=0.7, return_logprobs=True, u=None)))
    add("sample16_rows", [(3, 40)], lambda s: (dict(x=tensor(bf16, *s), u=0.5, top_k=5, top_p=0.9, min_p=0.1, temperature=0.7, return_logprobs=True), {}))
    add("logprobs16_rows", nd, lambda s: (dict(x=tensor(bf16, *s), ids=tensor(i64, *s[:-1])),
                                          dict(side, temperature=0.7, return_ranks=True, return_lse=True, ids=lambda: tensor(i32, *s[:-1], 40))))
    add("top_logprobs16_rows", [(2, 3, 40)], lambda s: (dict(x=tensor(bf16, *s), n=4), dict(side, temperature=0.7, n=36)))
    # ---- the run units; in place where that is allowed (GPUUnique, GPUReduceByKey) and where it is refused
    optional = lambda s: [True, lambda: tensor(i32, *s)]   # noqa: E731
    add("GPURunLength", flat, lambda s: (dict(d_keys=tensor(i32, *s)), dict(common, counts=optional(s), starts=optional(s), out=lambda: tensor(i32, *s))))
    add("GPUUnique", flat, lambda s: (dict(d_keys=tensor(i32, *s)), dict(common, counts=optional(s), first=optional(s), inverse=optional(s), descending=True,
                                                                        key_type="uint32", out=lambda: tensor(i32, *s))))
    for name in ("GPUReduceRuns", "GPUReduceByKey"):
        add(name, flat, lambda s: (dict(d_keys=tensor(i64, *s), d_vals=tensor(f32, *s)),
                                   dict(common, op="max", counts=optional(s), out_keys=lambda: tensor(i64, *s), out_vals=lambda: tensor(f32, *s))))
    for name, keys, vals in (("GPURunLength", "out", None), ("GPUUnique", "out", None), ("GPUReduceRuns", "out_keys", "out_vals"), ("GPUReduceByKey", "out_keys", "out_vals"),
                             ("GPUTopK16Filter", "out", None), ("GPUTopP16Filter", "out", None), ("GPUSortRows16", "out", None)):
        d_keys = tensor(bf16, 3, 40) if "16" in name else tensor(i32, 8)
        kwargs = dict(d_keys=d_keys, **{keys: d_keys})
        kwargs.update({"GPUTopK16Filter": dict(d_k=tensor(i32, 3), key_type="bfloat16"), "GPUTopP16Filter": dict(d_p=tensor(f32, 3)),
                       "GPUSortRows16": dict(key_type="bfloat16")}.get(name, {}))
        if vals:
            kwargs["d_vals"] = kwargs[vals] = tensor(i32, 8)
        out.append(("in place", name, kwargs))
    # ---- the stage entries and the partitions
    add("BuildHistograms", flat, lambda s: (dict(d_keys=tensor(i32, *s), r=8, bit_group=1), {}))
    add("BuildOffsets", [(2, 256)], lambda s: (dict(d_hist=tensor(i32, *s), r=8), side))
    add("RankScatter", flat, lambda s: (dict(d_in=tensor(i32, *s), d_global=tensor(i32, 1, 256), r=8, bit_group=0), dict(d_vals=lambda: tensor(i32, *s))))
    add("DigitHistograms", flat, lambda s: (dict(d_keys=tensor(i32, *s), r=8), {}))
    add("MSBPartition", flat, lambda s: (dict(d_keys=tensor(i32, *s), msb_bits=2), side))
    add("ThresholdPartition", flat, lambda s: (dict(d_keys=tensor(i32, *s), thresholds=[1, 2, 1 << 32]), side))
    add("SplitterPartition", flat, lambda s: (dict(d_keys=tensor(i32, *s), splitters=[1, 2, 3]), side))
    return out


def trace(lsd, out):
    global SIDE
    import torch

    if torch.cuda.is_available():
        SIDE = torch.cuda.Stream()
    table = cases()
    lines = [f"# {len(table)} cases"]
    for label, name, kwargs in table:
        lines += run_case(lsd, label, name, kwargs)
    text = "\n".join(lines) + "\n"
    if out:
        with open(out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
    print(f"face_calls: {len(table)} cases, {sum(1 for l in lines if ' | raises ' in l)} of them raise", file=sys.stderr)


def host_time(lsd, launch=True, calls=2000, warmup=200):
    """wall microseconds per call, caller's workspace; ``launch``: the real library, else the recorder (the Python layer alone)"""
    import torch

    if not launch:
        rec = Recorder(REAL)
        rec.calls = type("Dropped", (), {"append": staticmethod(lambda call: None)})()
        lsd.api.lib = lambda: rec

    ws = tensor(torch.uint8, 64 << 20)
    x16 = torch.randn(8, 1024, device=DEVICE).to(torch.bfloat16)
    x32 = torch.randint(-(1 << 31), (1 << 31) - 1, (8, 1024), dtype=torch.int32, device=DEVICE)
    keys = torch.randint(0, 64, (1024,), dtype=torch.int32, device=DEVICE)
    subjects = {"GPUKth16 [8,1024] bfloat16": lambda: lsd.GPUKth16(x16, 511, key_type="bfloat16", workspace=ws),
                "GPUTopK [8,1024] int32": lambda: lsd.GPUTopK(x32, 8, key_type="int32", workspace=ws),
                "GPUUnique 1024 int32": lambda: lsd.GPUUnique(keys, workspace=ws)}
    for label, call in subjects.items():
        for _ in range(warmup):
            call()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            call()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        print(f"{label}{'' if launch else ' (no launch)'}: {(t1 - t0) / calls * 1e6:.2f} us/call")


def main():
    global REAL
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout whose package is imported")
    ap.add_argument("--out", help="write the trace here instead of standard output")
    ap.add_argument("--time", action="store_true", help="measure host time per call instead")
    ap.add_argument("--no-launch", action="store_true", help="with --time: behind the recorder, so that only the Python layer is timed")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch  # noqa: F401  (before the library is loaded, as in the tests and bench.py: one HIP runtime in the process, torch's)

    import lsdradixsort_amd as lsd

    assert os.path.abspath(lsd.__file__).startswith(os.path.abspath(args.tree)), lsd.__file__
    REAL = lsd.lib()
    if args.time:
        host_time(lsd, launch=not args.no_launch)
    else:
        trace(lsd, args.out)


REAL = None

if __name__ == "__main__":
    main()
