"""Recording the package's C calls made under chosen methods of a class, for the launch-trace tests
(tests/test_backbone_trace_gpu.py, tests/test_head_trace_gpu.py).  A plain helper module.

What a trace line holds: the entry point's name, the fields of a ConvDesc argument, every integer and float argument, whether
each pointer argument is null (by the argument types of _lib.SIGNATURES), and the stream the call is queued on as an ordinal by
first appearance.  Pointer VALUES are not recorded: addresses depend on allocation order, which may change.
mvg_set_scratch / mvg_scratch_bytes are left out: whether a stream's workspace is already registered depends on what ran
earlier in the process.

A golden file holds, per case, a sha256 of the trace, the number of calls and the count per entry point."""
import contextlib
import ctypes as C
import hashlib
from collections import Counter

import torch

from rot_mvgaze_amd import _lib, ops

UNRECORDED = ("mvg_set_scratch", "mvg_scratch_bytes")


class Recorder:
    """The proxy that stands in for the loaded library: every mvg_* call made while ``depth`` > 0 becomes one trace line."""

    def __init__(self, real):
        self.real, self.depth, self.lines, self.streams, self.fns = real, 0, [], {}, {}

    def __getattr__(self, name):
        fn = self.fns.get(name)
        if fn is None:
            real_fn = getattr(self.real, name)
            if not name.startswith("mvg_") or name in UNRECORDED:
                fn = real_fn
            else:
                argtypes = _lib.SIGNATURES[name][1]

                def fn(*args, _real=real_fn, _name=name, _types=argtypes):
                    if self.depth > 0:
                        self.lines.append(self.describe(_name, _types, args))
                    return _real(*args)
            self.fns[name] = fn
        return fn

    def describe(self, name, argtypes, args):
        assert len(args) == len(argtypes), name
        parts = [name]
        for t, a in zip(argtypes, args):
            if t is _lib._D:
                d = a._obj                                           # C.byref(desc)
                parts.append("desc(" + ",".join(str(getattr(d, f)) for f, _ in _lib.ConvDesc._fields_) + ")")
            elif t is _lib._P:
                v = a.value if isinstance(a, C.c_void_p) else a
                parts.append("null" if not v else "ptr")
            elif t in (_lib._I, _lib._I64, C.c_int32, C.c_size_t, C.c_uint64):
                parts.append(str(int(a)))
            elif t is _lib._F:
                parts.append(repr(float(a)))
            else:                                                    # a host array or an out-parameter
                parts.append("null" if a is None else "ref")
        handle = torch.cuda.current_stream().cuda_stream
        parts.append("stream%d" % self.streams.setdefault(handle, len(self.streams)))
        return " ".join(parts)


_active = []                     # the Recorder of the record() call that is running, if any


@contextlib.contextmanager
def muted():
    """Inside record(): calls made in this block are left out of the trace."""
    held = [(rec, rec.depth) for rec in _active]
    for rec, _ in held:
        rec.depth = -(1 << 30)
    try:
        yield
    finally:
        for rec, depth in held:
            rec.depth = depth


def record(cls, methods, run):
    """Call run() with ops.lib replaced by a Recorder that is switched on while any of ``cls``'s ``methods`` is on the stack.
    Returns (trace lines, what run() returned)."""
    rec = Recorder(_lib.lib())
    _active.append(rec)
    saved_lib, saved = ops.lib, {n: getattr(cls, n) for n in methods}

    def switched(orig):
        def method(self, *a, **kw):
            rec.depth += 1
            try:
                return orig(self, *a, **kw)
            finally:
                rec.depth -= 1
        return method
    ops.lib = lambda: rec
    for n, orig in saved.items():
        setattr(cls, n, switched(orig))
    try:
        result = run()
    finally:
        _active.remove(rec)
        ops.lib = saved_lib
        for n, orig in saved.items():
            setattr(cls, n, orig)
    return rec.lines, result


def summarise(lines):
    counts = Counter(l.split(" ", 1)[0] for l in lines)
    return hashlib.sha256("\n".join(lines).encode()).hexdigest(), len(lines), dict(sorted(counts.items()))


def golden_row(name, lines):
    digest, n, counts = summarise(lines)
    return f"{name} {digest} {n} " + ",".join(f"{k}={v}" for k, v in counts.items())


def read_golden(path):
    golden = {}
    with open(path) as f:
        for line in f:
            if line.strip() and not line.startswith("#"):
                name, digest, n, counts = line.split()
                golden[name] = (digest, int(n), {k: int(v) for k, v in (kv.split("=") for kv in counts.split(","))})
    return golden


def assert_matches_golden(name, lines, golden, tool):
    """The trace of ``name`` against its golden entry; on a mismatch says which counts moved."""
    digest, n, counts = summarise(lines)
    want_digest, want_n, want_counts = golden[name]
    moved = {k: (want_counts.get(k, 0), counts.get(k, 0)) for k in sorted(set(counts) | set(want_counts))
             if counts.get(k, 0) != want_counts.get(k, 0)}
    assert not moved, f"{name}: launches per entry point moved (recorded, now): {moved}"
    assert n == want_n
    assert digest == want_digest, (f"{name}: the same {n} calls per entry point, but their order, arguments or streams differ: "
                                   f"diff the output of {tool} --dump DIR on the two commits")


def write_or_dump(argv, names, trace, golden_file, tool):
    """The command line of a trace test module: --write rewrites the golden file, --dump DIR writes the full traces."""
    import os
    if len(argv) == 2 and argv[0] == "--dump":
        os.makedirs(argv[1], exist_ok=True)
    elif argv != ["--write"]:
        raise SystemExit(f"usage: {tool} --write | --dump DIR")
    rows = []
    for name in names:
        lines = trace(name)
        rows.append(golden_row(name, lines))
        print(*rows[-1].split(" ")[:3], flush=True)
        if argv[0] == "--dump":
            with open(os.path.join(argv[1], name + ".txt"), "w") as f:
                f.write("\n".join(lines) + "\n")
    if argv[0] == "--write":
        with open(golden_file, "w") as f:
            f.write(f"# case sha256(trace) calls entry=count,...   (python tests/{tool} --write)\n")
            f.write("\n".join(rows) + "\n")
