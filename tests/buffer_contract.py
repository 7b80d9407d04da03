"""The workspace and output contract of a launcher, checked without tolerances ("Buffers").

A launcher of the C ABI is given buffers of EXACTLY the documented size, each between two guard regions, and is run three times
over outputs and scratch that hold zeros, the leftovers of another problem, and 0xFF bytes (NaN as fp32 / fp64, -1 as int32 /
int64).  The contract holds when every run returns 0, no guard byte changes, no read-only input changes, and the outputs of the
three runs are the same bits: a launcher that reads a word of scratch before writing it, accumulates into an output it never
cleared or leaves an output element unwritten cannot pass all three.

``device=None`` keeps every buffer in host memory (numpy): tests/test_buffer_contract_host.py runs the checker itself against
stand-in launchers with planted defects.  On the GPU the buffers are torch uint8 tensors and ``launch`` calls the library.
A plain module: imported by the two test files, no fixtures, no pytest hooks.
"""
import numpy as np

GUARD_BYTES = 4096
GUARD_FILL = 0xA5

_NP = {"f64": np.float64, "f32": np.float32, "i32": np.int32, "i64": np.int64, "u8": np.uint8}


class ContractError(AssertionError):
    """A launcher broke the buffer contract; the message names the buffer and the element."""


class Arena:
    """guard | payload | guard in one uint8 allocation.  The payload is exactly ``nbytes`` long and starts at an address that is
    a multiple of ``align``; the guards (>= 4096 bytes of 0xA5 each) touch it on both sides, so one element before the first or
    after the last lands in a guard."""

    def __init__(self, nbytes, align=16, device=None, name="buffer"):
        nbytes, align = int(nbytes), int(align)
        if nbytes < 0 or align < 1 or align & (align - 1):
            raise ValueError(f"Arena({nbytes}, {align}): a size >= 0 and a power-of-two alignment")
        self.name, self.nbytes, self.align, self.device = name, nbytes, align, device
        total = 2 * GUARD_BYTES + nbytes + align
        if device is None:
            self.raw = np.empty(total, dtype=np.uint8)
            base = self.raw.ctypes.data
        else:
            import torch
            self.raw = torch.empty(total, dtype=torch.uint8, device=device)
            base = self.raw.data_ptr()
        self.offset = GUARD_BYTES + (-(base + GUARD_BYTES)) % align
        self.ptr = base + self.offset
        self.raw[:] = GUARD_FILL
        self.payload = self.raw[self.offset:self.offset + nbytes]

    # ---- contents
    def fill(self, byte):
        self.payload[:] = int(byte)
        return self

    def write(self, array):
        """Host array (any dtype) -> payload; the byte counts must agree."""
        b = np.ascontiguousarray(array).reshape(-1).view(np.uint8)
        if b.size != self.nbytes:
            raise ValueError(f"{self.name}: {b.size} bytes for a payload of {self.nbytes}")
        if self.device is None:
            self.payload[:] = b
        elif b.size:
            import torch
            self.payload.copy_(torch.from_numpy(b.copy()))
        return self

    def host(self, kind="u8"):
        """A host COPY of the payload as ``kind`` elements (a trailing part shorter than one element is dropped)."""
        b = self.payload.copy() if self.device is None else self.payload.cpu().numpy().copy()     # (.cpu() of a host tensor is the tensor)
        item = np.dtype(_NP[kind]).itemsize
        return b[:b.size // item * item].view(_NP[kind])

    def _view(self, kind):
        item = np.dtype(_NP[kind]).itemsize
        p = self.payload[:self.nbytes // item * item]
        if self.device is None:
            return p.view(_NP[kind])
        import torch
        return p.view({"f64": torch.float64, "f32": torch.float32, "i32": torch.int32, "i64": torch.int64}[kind])

    def f64(self):
        return self._view("f64")

    def f32(self):
        return self._view("f32")

    def i32(self):
        return self._view("i32")

    def i64(self):
        return self._view("i64")

    # ---- guards
    def intact(self):
        """True while both guards hold 0xA5 everywhere (compared where the buffer lives; one scalar crosses to the host)."""
        front, back = self.raw[:self.offset], self.raw[self.offset + self.nbytes:]
        return bool((front == GUARD_FILL).all()) and bool((back == GUARD_FILL).all())

    def damage(self):
        """"" when intact, else where the first damaged guard byte lies relative to the payload."""
        if self.intact():
            return ""
        raw = self.raw if self.device is None else self.raw.cpu().numpy()
        out = []
        front = np.flatnonzero(raw[:self.offset] != GUARD_FILL)
        back = np.flatnonzero(raw[self.offset + self.nbytes:] != GUARD_FILL)
        if front.size:
            out.append(f"{front.size} byte(s) BEFORE the payload changed, the nearest {self.offset - int(front[-1])} byte(s) in front of "
                       f"element 0")
        if back.size:
            out.append(f"{back.size} byte(s) AFTER the payload changed, the first at byte {self.nbytes + int(back[0])} "
                       f"(payload is {self.nbytes} bytes)")
        return "; ".join(out)


class Buf:
    """An output or scratch buffer of ``count`` elements of ``kind`` ("f64", "f32", "i32", "i64", "u8") at ``align`` bytes.
    ``init``: a host array of ``count`` elements the buffer is loaded with before every run instead of the fill (an operand that is
    updated in place); ``init_mask`` (bool [count]): only those elements are loaded, the others get the fill (the pad columns of a
    pitched matrix)."""

    def __init__(self, kind, count, align=16, init=None, init_mask=None):
        self.kind, self.count, self.align = kind, int(count), int(align)
        self.nbytes = self.count * np.dtype(_NP[kind]).itemsize
        self.init = None if init is None else np.ascontiguousarray(init, dtype=_NP[kind]).reshape(-1)
        self.init_mask = None if init_mask is None else np.asarray(init_mask, dtype=bool).reshape(-1)


def _load(arena, buf, init, byte):
    """Bring an output / scratch arena to its state before a run: ``init`` (possibly shorter than the buffer: another problem's
    operand) where the buffer has one, the fill ``byte`` elsewhere (None: left as it is)."""
    if init is None:
        if byte is not None:
            arena.fill(byte)
        return
    init = np.ascontiguousarray(init, dtype=_NP[buf.kind]).reshape(-1)
    cur = arena.host(buf.kind) if byte is None else np.full(buf.nbytes, byte, dtype=np.uint8).view(_NP[buf.kind])
    if buf.init_mask is not None and init.size == buf.count:
        cur[buf.init_mask] = init[buf.init_mask]
    else:
        cur[:init.size] = init
    arena.write(cur)


def _sync(device):
    """Wait for the launches on a GPU; nothing to wait for on host buffers (numpy, or torch's "cpu")."""
    if device is not None and str(device).startswith("cuda"):
        import torch
        torch.cuda.synchronize()


def _bits(a):
    """Integer view of a host array, so that NaN compares equal to NaN."""
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def _first_diff(a, b):
    d = np.flatnonzero(_bits(a) != _bits(b))
    return (int(d[0]), int(d.size)) if d.size else (None, 0)


def _index_mask(spec, count):
    m = np.zeros(count, dtype=bool)
    if spec is not None:
        spec = np.asarray(spec).reshape(-1)
        if spec.dtype == bool:
            if spec.size != count:
                raise ValueError(f"a mask of {spec.size} elements for a buffer of {count}")
            m |= spec
        else:
            m[spec.astype(np.int64)] = True
    return m


class ContractResult:
    """``outputs[name]`` / ``scratch[name]``: host copies (typed) after the first run; ``arenas``: every arena by name."""

    def __init__(self, outputs, scratch, arenas):
        self.outputs, self.scratch, self.arenas = outputs, scratch, arenas


def run_contract(launch, inputs, outputs, scratch, other_inputs, *, device=None, align=None, unwritten=None, documented=None,
                 unspecified=(), other_launch=None, other_init=None, what="launcher"):
    """Run ``launch`` under the three fills and assert the contract.

    launch(bufs) -> return code.  ``bufs[name]`` is the Arena of that input, output or scratch buffer (``.ptr`` is the address to
    pass; ``.f64()`` ... are typed views).
    inputs        {name: host array}: read-only operands, each in an arena of exactly its size.
    outputs       {name: Buf}: compared bit for bit across the three runs.
    scratch       {name: Buf}: contents unspecified on entry and on return, of exactly the size the launcher's query gives.
    other_inputs  {name: host array}: another problem, run between the first and the second run so that the second starts from
                  its leftovers; ``other_launch`` when its shape (and so its call) differs -- it gets the same output and scratch
                  arenas and input arenas of its own sizes.  ``other_init`` {name: host array}: what an in-place operand holds
                  for that problem (no longer than the buffer).
    align         {name: bytes} where the header asks for more than 16.
    unwritten     {output name: indices or bool mask}: elements the header documents as NOT written; checked to keep what they
                  held before each run, and left out of the comparison.
    documented    {scratch name: indices or bool mask}: scratch elements whose contents on return the header documents; compared
                  across the runs like an output.
    unspecified   names of outputs whose contents on return the header leaves open (an operand that is "overwritten"): guards
                  only.
    Returns a ContractResult with the first run's outputs."""
    align, unwritten, documented = dict(align or {}), dict(unwritten or {}), dict(documented or {})
    kinds = {}

    def input_arenas(arrays):
        out = {}
        for name, a in arrays.items():
            a = np.ascontiguousarray(a)
            out[name] = Arena(a.nbytes, align.get(name, 16), device, name).write(a)
        return out

    ins, other_ins = input_arenas(inputs), input_arenas(other_inputs)
    work = {}
    for group in (outputs, scratch):
        for name, b in group.items():
            work[name] = Arena(b.nbytes, align.get(name, b.align), device, name)
            kinds[name] = b.kind
    masks = {name: _index_mask(unwritten.get(name), b.count) for name, b in outputs.items()}
    doc = {name: _index_mask(documented.get(name), scratch[name].count) for name in documented}

    def sync():
        _sync(device)

    def prepare(byte, inits=None):
        for group in (outputs, scratch):
            for name, b in group.items():
                _load(work[name], b, (inits or {}).get(name, b.init), byte)

    def snapshot():
        return {name: work[name].host(kinds[name]) for name in work}

    def check_run(label, fn, in_arenas, in_arrays, before):
        rc = fn({**in_arenas, **work})
        sync()
        if rc != 0:
            raise ContractError(f"{what}, {label}: return code {rc}")
        for name, arena in {**in_arenas, **work}.items():
            bad = arena.damage()
            if bad:
                role = "input" if name in in_arenas else "output" if name in outputs else "scratch"
                raise ContractError(f"{what}, {label}: {role} '{name}' was written outside its {arena.nbytes} bytes: {bad}")
        for name, a in in_arrays.items():
            a = np.ascontiguousarray(a)
            now = in_arenas[name].host("u8").view(a.dtype) if a.size else a.reshape(-1)
            i, n = _first_diff(a.reshape(-1), now)
            if i is not None:
                raise ContractError(f"{what}, {label}: read-only input '{name}' was modified: element {i} ({n} in all) is {now[i]!r}, "
                                    f"was {a.reshape(-1)[i]!r}")
        after = snapshot()
        for name, m in masks.items():
            if m.any():
                i, n = _first_diff(before[name][m], after[name][m])
                if i is not None:
                    e = int(np.flatnonzero(m)[i])
                    raise ContractError(f"{what}, {label}: output '{name}' element {e} is documented as not written but changed "
                                        f"({n} such element(s))")
        return after

    def compare(label_a, a, label_b, b, fills):
        for name in list(outputs) + list(doc):
            if name in unspecified:
                continue
            keep = ~masks[name] if name in outputs else doc[name]
            idx = np.flatnonzero(keep)
            i, n = _first_diff(a[name][keep], b[name][keep])
            if i is None:
                continue
            e = int(idx[i])
            role = "output" if name in outputs else "scratch (documented part)"
            item = a[name].dtype.itemsize
            never = fills is not None and all(
                bytes(_bits(x[name][e:e + 1]).tobytes()) == bytes([f]) * item for x, f in zip((a, b), fills))
            why = ("it was never written: it holds its fill after both runs" if never else
                   "the result depends on what the outputs or the scratch held before the call (a word read before it was "
                   "written, or an accumulation that does not start from zero)")
            raise ContractError(f"{what}: {role} '{name}' element {e} differs between the {label_a} run ({a[name][e]!r}) and the "
                                f"{label_b} run ({b[name][e]!r}), {n} element(s) in all: {why}")

    prepare(0x00)
    before = snapshot()
    first = check_run("0x00 fill", launch, ins, inputs, before)
    prepare(None, other_init)
    before = snapshot()
    check_run("other problem", other_launch or launch, other_ins, other_inputs, before)
    prepare(None)
    before = snapshot()
    stale = check_run("stale", launch, ins, inputs, before)
    compare("0x00-fill", first, "stale", stale, None)
    prepare(0xFF)
    before = snapshot()
    last = check_run("0xFF fill", launch, ins, inputs, before)
    compare("0x00-fill", first, "0xFF-fill", last, (0x00, 0xFF))
    arenas = {**ins, **work}
    return ContractResult({n: first[n] for n in outputs}, {n: first[n] for n in scratch}, arenas)


def run_zero_fill_only(launch, inputs, outputs, scratch, *, device=None, align=None, what="launcher"):
    """The part of the contract that needs no claim about uninitialised words: one run over zero-filled outputs and scratch of
    exactly the documented size, return code 0, guards intact, inputs unchanged.  For a launcher whose reads of scratch could not
    be established from its code (see the case's comment).  Returns a ContractResult."""
    align = dict(align or {})
    ins = {}
    for name, a in inputs.items():
        a = np.ascontiguousarray(a)
        ins[name] = Arena(a.nbytes, align.get(name, 16), device, name).write(a)
    work = {}
    for group in (outputs, scratch):
        for name, b in group.items():
            work[name] = Arena(b.nbytes, align.get(name, b.align), device, name)
            _load(work[name], b, b.init, 0x00)
    rc = launch({**ins, **work})
    _sync(device)
    if rc != 0:
        raise ContractError(f"{what}, 0x00 fill: return code {rc}")
    for name, arena in {**ins, **work}.items():
        bad = arena.damage()
        if bad:
            raise ContractError(f"{what}, 0x00 fill: '{name}' was written outside its {arena.nbytes} bytes: {bad}")
    for name, a in inputs.items():
        a = np.ascontiguousarray(a)
        if a.size:
            now = ins[name].host("u8").view(a.dtype)
            i, n = _first_diff(a.reshape(-1), now)
            if i is not None:
                raise ContractError(f"{what}, 0x00 fill: read-only input '{name}' was modified: element {i} ({n} in all)")
    kind = {**{n: b.kind for n, b in outputs.items()}, **{n: b.kind for n, b in scratch.items()}}
    return ContractResult({n: work[n].host(kind[n]) for n in outputs}, {n: work[n].host(kind[n]) for n in scratch}, {**ins, **work})
