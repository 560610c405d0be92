"""Shared pieces of the connected component and island removal tests (test_ccl_cpu.py, test_gpu_ccl.py): the
CPU oracle tests/ccl_oracle.c, the label patterns, the planted cases of the cleaning rule, and both restated in plain Python."""
import ctypes as C
from collections import deque

import numpy as np

from _helpers import c_oracle
from edt_cases import blocky_pair

RECORD = np.dtype([("label", "<i4"), ("reserved", "<i4"), ("voxels", "<i8"), ("first", "<i8"), ("box", "<i4", (6,))])
ROUND_FIELDS = ("components", "small", "resolved", "resolved_voxels", "unresolved", "unresolved_voxels")
PATTERNS = ["one", "nan", "checker", "corner_pair", "serpentine", "u", "random2", "random5", "blocky"]
# kernels_ccl.hip: a brick is 32 x 8 x 4 voxels
BX, BY, BZ = 32, 8, 4


class _Round(C.Structure):
    _fields_ = [(name, C.c_int64) for name in ROUND_FIELDS]


class _Report(C.Structure):
    _fields_ = [("rounds_run", C.c_int32), ("reserved", C.c_int32), ("round", _Round * 16), ("total", _Round)]


def report_dict(rep):
    row = lambda r: {k: int(getattr(r, k)) for k in ROUND_FIELDS}
    return {"rounds_run": int(rep.rounds_run), "rounds": [row(rep.round[r]) for r in range(rep.rounds_run)], "total": row(rep.total)}


class CclOracle:
    def __init__(self, tmpdir):
        L = c_oracle("ccl_oracle", tmpdir)
        P, I64, I32 = C.c_void_p, C.c_int64, C.c_int32
        L.occ_label.restype = I64
        L.occ_label.argtypes = [P, I64, I64, I64, C.c_int, P, P, I64]
        L.occ_clean.restype = C.c_int
        L.occ_clean.argtypes = [P, I64, I64, I64, I32, I32, I32, P, P]
        self.L = L

    def label(self, labels, conn):
        """(the component map uint32 (nz, ny, nx), the records in key order)"""
        v = np.ascontiguousarray(labels, np.float32)
        nz, ny, nx = v.shape
        comp = np.empty(v.shape, np.uint32)
        n = self.L.occ_label(v.ctypes.data, nx, ny, nz, conn, comp.ctypes.data, None, 0)
        assert n >= 0
        rec = np.zeros(max(n, 1), RECORD)
        assert self.L.occ_label(v.ctypes.data, nx, ny, nz, conn, comp.ctypes.data, rec.ctypes.data, n) == n
        return comp, rec[:n].copy()

    def clean(self, labels, min_voxels=8, connectivity=6, rounds=4):
        """(the cleaned labels float32, the report as report_dict gives it)"""
        v = np.ascontiguousarray(labels, np.float32)
        nz, ny, nx = v.shape
        out = np.empty(v.shape, np.float32)
        rep = _Report()
        assert self.L.occ_clean(v.ctypes.data, nx, ny, nz, min_voxels, connectivity, rounds, out.ctypes.data, C.byref(rep)) == 0
        return out, report_dict(rep)


def same_records(got, want):
    assert got.dtype == RECORD and len(got) == len(want), (len(got), len(want))
    for name in RECORD.names:
        assert np.array_equal(got[name], want[name]), (name, np.nonzero((got[name] != want[name]).reshape(len(got), -1).any(1))[0][:5])


def same_bits(got, want):
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got.view(np.uint32) != want.view(np.uint32)).sum())


# ---- the label patterns ------------------------------------------------------------------------------------------------------------
def serpentine(shape):
    """label 2 on a path one voxel wide through the whole volume, label 0 around it: every other row of every other plane in full,
    neighbouring rows joined at alternating ends, neighbouring planes likewise; the path starts at voxel 0, its smallest index"""
    nz, ny, nx = shape
    v = np.zeros(shape, np.float32)
    rows = list(range(0, ny, 2))
    end = (rows[-1], nx - 1 if (len(rows) - 1) % 2 == 0 else 0)   # where a plane's path ends when it starts at (0, 0)
    for c, z in enumerate(range(0, nz, 2)):
        for r, y in enumerate(rows):
            v[z, y, :] = 2
            if y + 2 < ny:
                v[z, y + 1, nx - 1 if r % 2 == 0 else 0] = 2
        if z + 2 < nz:                                            # the planes are walked forth and back: joined at alternating ends
            v[z + 1, end[0] if c % 2 == 0 else 0, end[1] if c % 2 == 0 else 0] = 2
    return v


def u_shape(shape):
    """label 3 as a U whose arms lie in one brick and join only in the next, along the first axis that has room for it"""
    nz, ny, nx = shape
    v = np.zeros(shape, np.float32)
    if nx > BX + 1 and ny >= 6:
        z = min(1, nz - 1)
        v[z, 1, 10:BX + 2] = v[z, 5, 10:BX + 2] = 3
        v[z, 1:6, BX + 1] = 3
    elif ny > BY + 1 and nx >= 4:
        z = min(1, nz - 1)
        v[z, 2:BY + 2, 1] = v[z, 2:BY + 2, 3] = 3
        v[z, BY + 1, 1:4] = 3
    elif nz > BZ + 1 and nx >= 4:
        v[1:BZ + 2, 0, 1] = v[1:BZ + 2, 0, 3] = 3
        v[BZ + 1, 0, 1:4] = 3
    return v


def corner_pair(shape):
    """label 5 at two voxels that touch only at a corner, across the brick corner (31, 7, 3) - (32, 8, 4) where the volume reaches it"""
    nz, ny, nx = shape
    v = np.zeros(shape, np.float32)
    x, y, z = min(BX - 1, nx - 2), min(BY - 1, ny - 2), min(BZ - 1, nz - 2)
    if min(x, y, z) < 0:          # a line or a sheet has no corner contact: one voxel
        v[0, 0, 0] = 5
        return v
    v[z, y, x] = v[z + 1, y + 1, x + 1] = 5
    return v


def pattern(shape, name, seed=0):
    """float32 (nz, ny, nx)"""
    rng = np.random.default_rng(seed + 17 * shape[0] + 5 * shape[1] + shape[2])
    z, y, x = np.meshgrid(*(np.arange(s) for s in shape), indexing="ij")
    if name == "one":
        return np.ones(shape, np.float32)
    if name == "nan":
        return np.full(shape, np.nan, np.float32)
    if name == "checker":
        return ((x + y + z) % 2 + 1).astype(np.float32)
    if name == "corner_pair":
        return corner_pair(shape)
    if name == "serpentine":
        return serpentine(shape)
    if name == "u":
        return u_shape(shape)
    if name == "random2":
        return rng.integers(1, 3, shape).astype(np.float32)
    if name == "random5":
        v = np.array([0, 1, 2, 7, 65535], np.float32)[rng.integers(0, 5, shape)]
        at = rng.random(shape) < 0.03
        v[at] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), int(at.sum()))
        return np.ascontiguousarray(v)
    assert name == "blocky"
    return blocky_pair(shape)[0]


# ---- the contract in plain Python ------------------------------------------------------------------------------------------------------
def _neighbours(conn):
    return [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if (dx, dy, dz) != (0, 0, 0) and (conn == 26 or abs(dx) + abs(dy) + abs(dz) == 1)]


def label_python(labels, conn):
    """the component map and the records by a breadth-first search over Python integers"""
    v = np.asarray(labels, np.float32)
    nz, ny, nx = v.shape
    flat = [float(f) for f in v.reshape(-1)]
    fin = [bool(b) for b in np.isfinite(v).reshape(-1)]
    comp = [0] * len(flat)
    rec = []
    steps = _neighbours(conn)
    for start in range(len(flat)):
        if comp[start] or not fin[start]:
            continue
        number = len(rec) + 1
        comp[start] = number
        todo = deque([start])
        xs, ys, zs = [], [], []
        while todo:
            i = todo.popleft()
            x, y, z = i % nx, i // nx % ny, i // (nx * ny)
            xs.append(x), ys.append(y), zs.append(z)
            for dx, dy, dz in steps:
                ax, ay, az = x + dx, y + dy, z + dz
                if 0 <= ax < nx and 0 <= ay < ny and 0 <= az < nz:
                    j = (az * ny + ay) * nx + ax
                    if not comp[j] and fin[j] and flat[j] == flat[start]:
                        comp[j] = number
                        todo.append(j)
        rec.append((int(flat[start]), 0, len(xs), start, (min(xs), max(xs), min(ys), max(ys), min(zs), max(zs))))
    return np.array(comp, np.uint32).reshape(v.shape), np.array(rec, RECORD) if rec else np.zeros(0, RECORD)


def clean_python(labels, min_voxels=8, connectivity=6, rounds=4):
    """the rounds in plain Python on label_python's components: (the cleaned labels, the report)"""
    cur = np.array(labels, np.float32)
    nz, ny, nx = cur.shape
    rep = {"rounds_run": 0, "rounds": [], "total": dict.fromkeys(ROUND_FIELDS, 0)}
    for r in range(rounds):
        comp, rec = label_python(cur, connectivity)
        comp = comp.reshape(-1)
        flat = cur.reshape(-1)
        row = dict.fromkeys(ROUND_FIELDS, 0)
        row["components"] = len(rec)
        out = cur.copy().reshape(-1)
        members = {}
        for i, k in enumerate(comp):
            if k and rec["voxels"][k - 1] < min_voxels:
                members.setdefault(int(k), []).append(i)
        for k in sorted(members):
            votes = {}
            for i in members[k]:
                x, y, z = i % nx, i // nx % ny, i // (nx * ny)
                for dx, dy, dz in _neighbours(6):
                    ax, ay, az = x + dx, y + dy, z + dz
                    if 0 <= ax < nx and 0 <= ay < ny and 0 <= az < nz:
                        j = (az * ny + ay) * nx + ax
                        if comp[j] and rec["voxels"][comp[j] - 1] >= min_voxels:
                            votes[int(flat[j])] = votes.get(int(flat[j]), 0) + 1
            row["small"] += 1
            if votes:
                winner = min(votes, key=lambda l: (-votes[l], l))
                row["resolved"] += 1
                row["resolved_voxels"] += len(members[k])
                out[members[k]] = winner
            else:
                row["unresolved"] += 1
                row["unresolved_voxels"] += len(members[k])
        cur = out.reshape(cur.shape)
        rep["rounds"].append(row)
        rep["rounds_run"] = r + 1
        t = rep["total"]
        t["components"] = rep["rounds"][0]["components"]
        t["resolved"] += row["resolved"]
        t["resolved_voxels"] += row["resolved_voxels"]
        t["small"], t["unresolved"], t["unresolved_voxels"] = row["small"], row["unresolved"], row["unresolved_voxels"]
        if row["resolved"] == 0:
            break
    return cur, rep


# ---- the planted cases of the cleaning rule ----------------------------------------------------------------------------------------------
def nan_payload():
    return np.array([0x7fc12345], np.uint32).view(np.float32)[0]


def planted():
    """name -> (labels, parameters): every clause of the rule on a volume of its own, 9 x 10 x 12 voxels but for the nested pair's sheet"""
    shape = (9, 10, 12)
    cases = {}
    v = np.full(shape, 1, np.float32)
    v[4, 4, 4:7] = 6                                  # an island of 3 inside label 1
    cases["island"] = (v, {})
    v = np.full(shape, 3, np.float32)
    v[2, 3, 4] = 0                                    # a pinhole of background inside label 3
    v[0, 0, 0] = nan_payload()                        # an unlabelled voxel keeps its bits
    cases["pinhole"] = (v, {})
    v = np.full(shape, 2, np.float32)
    v[:, :, 6:] = 5
    v[4, 4, 5:7] = 9                                  # two voxels astride the border of 2 and 5: five faces each
    cases["tie"] = (v, {})
    v = np.full(shape, 4, np.float32)
    v[0, 0, 0:2] = 8                                  # at the volume's corner: the outside faces cast no vote
    cases["corner"] = (v, {})
    v = np.full(shape, 1, np.float32)
    v[3:6, 3:6, 3:6] = np.nan
    v[4, 4, 4] = 7                                    # walled in by unlabelled voxels: unresolved, keeps its bits
    cases["walled_nan"] = (v, {})
    v = ((np.indices(shape).sum(0)) % 2 + 1).astype(np.float32)   # nothing but small components: nobody votes
    cases["all_small"] = (v, {})
    v = np.full(shape, 1, np.float32)
    v[3:6, 3:6, 3:6] = 2                              # 27 voxels of 2 ...
    v[4, 4, 4] = 3                                    # ... around one of 3: 26 are kept at 8, the centre is small
    v[2, 3:5, 3] = 4
    cases["kept_inner"] = (v, {})
    cases["nested"] = (nested(), {})
    cases["nested_r1"] = (nested(), {"rounds": 1})
    v = np.full(shape, 1, np.float32)
    v[4, 4, 4] = 6
    v[5, 5, 5] = 6                                    # a corner pair of 6: one component of 2 under 26, two of 1 under 6
    v[4, 4, 5] = 2                                    # a face neighbour of the first, small itself: no vote from it
    cases["faces_only_26"] = (v, {"connectivity": 26, "min_voxels": 2})
    cases["faces_only_6"] = (v, {"connectivity": 6, "min_voxels": 2})
    v = np.full(shape, 1, np.float32)
    v[0, 0:2, 0:2] = 6
    v[0, 0, 0] = 2                                    # its faces see 6, 6 and 1, its edges 6, 1 and 1, its corner 1: only faces make it 6
    cases["faces_decide"] = (v, {"connectivity": 26, "min_voxels": 2})
    return cases


def nested():
    """a sheet: 3 voxels of label 3 on the sheet's edge inside the 5 voxels of label 5 that are all their face neighbours, inside a
    large region of label 1.  At min_voxels 8 both are small: the first round can resolve only the outer voxels, the second the inner"""
    v = np.full((1, 10, 12), 1, np.float32)
    v[0, 0, 3:8] = 5
    v[0, 1, 4:7] = 5
    v[0, 0, 4:7] = 3
    return v
