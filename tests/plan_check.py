"""An independent check of the general graph planner's buffer assignment (stage 7).

`plan_dump --lifetimes` prints, behind each plan, the virtual buffer every view had before assignBuffers renamed it.
This module parses that text and holds it against the rules of the design text, restated here from the text and not
from assignBuffers' code.  A launch touches a virtual buffer through any of its views; the last view of a launch is
its output (a write), every other one a read.  A virtual buffer lives from its first write to its last touch, and the
virtual buffers of policy, value and draw live to the end.

  R1  two virtual buffers on one physical buffer have disjoint intervals [first write, last touch]; intervals that
      meet in one launch collide, so a launch's output never shares a physical buffer with anything the launch reads
  R2  every read of a virtual buffer follows a write to it by an earlier launch (the input planes, buffer -1, excepted)
  R3  no launch after the producer of policy, value or draw writes the physical buffer of that output
  R4  every view fits its row (offset + C <= stride), every tenant fits its physical buffer (its stride at most
      bufSpatialStride for a spatial tenant, bufFlatStride for a flat one, where a line tensor counts lines * stride;
      an also-flat stride at most bufFlatStride), and a line view lies inside its tenant
  R5  activationBytesPerPosition = 4 (planeStride 81 + sum over the buffers of max(81 bufSpatialStride, bufFlatStride))

`check` returns the violations as (rule, message) pairs.  `allocate` is a short restatement of the first-fit
allocation, with the option of ignoring one view field: tests/test_plan_lifetimes.py uses it to show that every field
has a topology in which forgetting the field makes two live tensors collide."""
import copy
import os
import re
import subprocess
import sys
from dataclasses import dataclass, field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_DUMP = os.path.join(ROOT, "nshogi-engine_amd", "csrc", "plan_dump")
OUTPUTS = ("policy", "value", "draw")


@dataclass
class Ref:
    """One view of a launch: its field name, its virtual buffer and the renamed view."""
    field: str
    virt: int
    phys: int
    stride: int
    offset: int
    C: int
    spatial: bool
    lines: int = 0
    line0: int = 0
    buf_lines: int = 0

    @property
    def used(self):  # a default view (no residual, no K / V ...) names no buffer and has no width
        return self.virt >= 0


@dataclass
class Virt:
    stride: int
    spatial: bool
    also_flat: int
    phys: int


@dataclass
class Plan:
    name: str = ""
    plane_stride: int = 0
    activation_bytes: int = 0
    buf_spatial: list = field(default_factory=list)
    buf_flat: list = field(default_factory=list)
    virts: list = field(default_factory=list)
    launches: list = field(default_factory=list)  # of lists of Ref, the output last
    names: list = field(default_factory=list)     # the launches' node names
    kinds: list = field(default_factory=list)     # ... and their LaunchKind
    outputs: list = field(default_factory=list)   # policy, value, draw

    def touches(self, ignore=None):
        """(launch, Ref, is_write) of every used view; an output view counts as a read at launch len(launches)."""
        for i, row in enumerate(self.launches):
            for k, r in enumerate(row):
                if r.used and r.field != ignore:
                    yield i, r, k == len(row) - 1
        for r in self.outputs:
            if r.used and r.field != ignore:
                yield len(self.launches), r, False

    def intervals(self, ignore=None):
        """{virtual: [first write, last touch]} (first write None: never written)."""
        iv = {}
        for i, r, write in self.touches(ignore):
            lo, hi = iv.get(r.virt, (None, -1))
            if write and lo is None:
                lo = i
            iv[r.virt] = (lo, max(hi, i))
        return iv


_VIEW = re.compile(r"(\w+):(-?\d+) v=(-?\d+)/(\d+)/(\d+)/(\d+)/([sf])(?:/L(\d+)@(\d+)/(\d+))?")


def _refs(text):
    out = []
    for m in _VIEW.finditer(text):
        f, virt, phys, stride, off, c, kind, ln, l0, bl = m.groups()
        out.append(Ref(f, int(virt), int(phys), int(stride), int(off), int(c), kind == "s", int(ln or 0), int(l0 or 0), int(bl or 0)))
    return out


def parse(text):
    """The plans of a `plan_dump --lifetimes` output, in order.  A refused model raises."""
    plans, p = [], None
    for line in text.splitlines():
        if line.startswith("== "):
            p = Plan(name=line[3:].split()[0])
            plans.append(p)
        elif line.startswith("ERROR"):
            raise ValueError(f"{p.name}: {line}")
        elif line.startswith("numChannels="):
            p.plane_stride = int(re.search(r"planeStride=(\d+)", line).group(1))
            p.activation_bytes = int(re.search(r"activationBytesPerPosition=(\d+)", line).group(1))
        elif line.startswith("bufSpatialStride"):
            p.buf_spatial = [int(t) for t in line.split()[1:]]
        elif line.startswith("bufFlatStride"):
            p.buf_flat = [int(t) for t in line.split()[1:]]
        elif line.startswith("#"):
            p.names.append(re.search(r"name=(\S*)", line).group(1))
            p.kinds.append(int(re.search(r"kind=(\d+)", line).group(1)))
        elif re.match(r"V\d+ ", line):
            m = re.match(r"V(\d+) stride=(\d+) spatial=(\d) alsoFlat=(\d+) phys=(-?\d+)", line)
            assert int(m.group(1)) == len(p.virts), line
            p.virts.append(Virt(int(m.group(2)), m.group(3) == "1", int(m.group(4)), int(m.group(5))))
        elif re.match(r"L\d+ ", line):
            assert int(line[1:].split()[0]) == len(p.launches), line
            row = _refs(line)
            assert row and row[-1].field == "out", line
            p.launches.append(row)
        elif line.startswith("LO "):
            p.outputs = _refs(line)
            assert [r.field for r in p.outputs] == list(OUTPUTS), line
    for p in plans:
        assert p.launches and len(p.launches) == len(p.names) and len(p.outputs) == 3, p.name
    return plans


def dump(paths, planes=86):
    """Runs plan_dump --lifetimes on model files and parses its output (builds the tool first where it is missing)."""
    if not os.path.exists(PLAN_DUMP):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    args = [PLAN_DUMP, "--lifetimes"]
    for path in paths:
        n = planes.get(os.path.basename(path), 86) if isinstance(planes, dict) else planes
        args += ["--planes", str(n), str(path)]
    return parse(subprocess.run(args, check=True, capture_output=True, text=True).stdout)


def check(p):
    """The violations of R1-R5 in plan p: a list of (rule, message)."""
    bad = []
    nl = len(p.launches)
    iv = p.intervals()
    every = [(i, r, w) for i, r, w in p.touches()]

    # R2 (and the renaming itself: one virtual buffer, one physical buffer)
    for i, r, write in every:
        if r.virt >= len(p.virts):
            bad.append(("R2", f"launch {i} {r.field}: virtual buffer {r.virt} does not exist"))
            continue
        if r.phys != p.virts[r.virt].phys or r.phys < 0 or r.phys >= len(p.buf_spatial):
            bad.append(("R1", f"launch {i} {r.field}: virtual {r.virt} is renamed to {r.phys}, its buffer is {p.virts[r.virt].phys}"))
        if not write:
            first = iv[r.virt][0]
            if first is None or first >= i:
                bad.append(("R2", f"launch {i} {r.field} reads virtual {r.virt} before a launch has written it (first write: {first})"))

    # R1
    tenants = {}
    for v, (lo, hi) in iv.items():
        if lo is not None and v < len(p.virts):
            tenants.setdefault(p.virts[v].phys, []).append((lo, hi, v))
    for phys, ts in tenants.items():
        ts.sort()
        for a in range(len(ts)):
            for b in range(a + 1, len(ts)):
                if ts[b][0] <= ts[a][1]:
                    bad.append(("R1", f"physical {phys}: virtual {ts[a][2]} lives over launches {ts[a][:2]} and virtual {ts[b][2]} over {ts[b][:2]}"))

    # R3
    for o in p.outputs:
        if not o.used:
            bad.append(("R3", f"{o.field} names no activation buffer"))
            continue
        writes = [i for i, r, w in every if w and r.virt == o.virt]
        if not writes:
            continue  # R2 has it
        for i, r, w in every:
            if w and i > max(writes) and r.phys == o.phys:
                bad.append(("R3", f"launch {i} writes physical {r.phys}, which holds {o.field} since launch {max(writes)}"))
        if iv[o.virt][1] != nl:
            bad.append(("R3", f"{o.field} is not live to the end"))

    # R4
    for i, r, _ in every:
        if r.offset + r.C > r.stride:
            bad.append(("R4", f"launch {i} {r.field}: offset {r.offset} + C {r.C} > stride {r.stride}"))
        if r.lines and r.virt < len(p.virts):
            if r.line0 + r.lines > r.buf_lines or r.buf_lines * r.stride > p.virts[r.virt].stride:
                bad.append(("R4", f"launch {i} {r.field}: lines {r.line0}+{r.lines} of {r.buf_lines} at stride {r.stride} in a tenant of {p.virts[r.virt].stride}"))
    for v, t in enumerate(p.virts):
        if v not in iv:
            continue
        if not 0 <= t.phys < len(p.buf_spatial) or len(p.buf_flat) != len(p.buf_spatial):
            bad.append(("R4", f"virtual {v}: physical {t.phys} is outside the stride tables"))
            continue
        room = p.buf_spatial[t.phys] if t.spatial else p.buf_flat[t.phys]
        if t.stride > room:
            bad.append(("R4", f"virtual {v} ({'spatial' if t.spatial else 'flat'} stride {t.stride}) exceeds physical {t.phys}'s {room}"))
        if t.also_flat > p.buf_flat[t.phys]:
            bad.append(("R4", f"virtual {v}'s also-flat stride {t.also_flat} exceeds physical {t.phys}'s bufFlatStride {p.buf_flat[t.phys]}"))

    # R5
    want = 4 * (p.plane_stride * 81 + sum(max(81 * s, f) for s, f in zip(p.buf_spatial, p.buf_flat)))
    if want != p.activation_bytes:
        bad.append(("R5", f"activationBytesPerPosition {p.activation_bytes}, the stride tables give {want}"))
    return bad


def rules(p):
    return sorted({rule for rule, _ in check(p)})


def allocate(p, ignore=None):
    """First fit, restated: walking the launches in order, an output that has no buffer yet takes the first free
    physical buffer that already has room for it, else the first free one, else a new one; a buffer is free again after
    the last launch that touches its tenant.  `ignore`: a view field (or output name) the lifetimes do not see.
    Returns a copy of p with the physical ids, the views and the stride tables of this allocation."""
    q = copy.deepcopy(p)
    last = {v: hi for v, (lo, hi) in q.intervals(ignore).items()}
    spatial, flat, free, phys = [], [], [], {}
    for i, row in enumerate(q.launches):
        v = row[-1].virt
        t = q.virts[v]
        if v not in phys:
            room = spatial if t.spatial else flat
            pick = next((k for k in range(len(free)) if free[k] and room[k] >= t.stride), None)
            if pick is None:
                pick = next((k for k in range(len(free)) if free[k]), None)
            if pick is None:
                pick = len(free)
                free.append(False)
                spatial.append(0)
                flat.append(0)
            free[pick] = False
            room[pick] = max(room[pick], t.stride)
            flat[pick] = max(flat[pick], t.also_flat)
            phys[v] = pick
        for w, k in phys.items():
            if last.get(w, -1) == i:
                free[k] = True
    for v, t in enumerate(q.virts):
        t.phys = phys.get(v, -1)
    for _, r, _ in q.touches():
        r.phys = q.virts[r.virt].phys
    q.buf_spatial, q.buf_flat = spatial, flat
    q.activation_bytes = 4 * (q.plane_stride * 81 + sum(max(81 * s, f) for s, f in zip(spatial, flat)))
    return q


def fields(p):
    """The view fields plan p reads a written tensor through (outputs included)."""
    return sorted({r.field for _, r, w in p.touches() if not w})
