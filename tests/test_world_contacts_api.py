"""The contact query of a world (rb_query_contacts, rb_query_contacts_dev;
World.query_contacts, query_contacts_device, WorldContacts): the entry points
are exported with the header's argument lists, the binding's argtypes match
them, a null handle is refused before any device call, WorldContacts.to_csr()
gives the CSR shape of World.contacts() on hand-made arrays (truncated rows and
-2 rows included), and the new kernels compile without scratch (no GPU here)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT

FUNCS = ["rb_query_contacts", "rb_query_contacts_dev"]
KERNELS = {"world_contacts_kernel", "world_contacts_boxes_kernel"}
EINVAL = -22
# a C parameter type -> the ctypes type the binding must give it
CTYPES = {"rb_world *": C.c_void_p, "int64_t": C.c_int64, "int32_t": C.c_int32, "int32_t *": C.c_void_p,
          "double *": C.c_void_p, "void *": C.c_void_p, "int64_t *": C.POINTER(C.c_int64)}


@pytest.fixture(scope="module")
def lib():
    path = os.path.join(PKG, "rbhip", "librbhip.so")
    if not os.path.exists(path):
        subprocess.run(["make", "-s", "-C", os.path.join(PKG, "csrc")], check=True)
    from rbhip import _lib
    return _lib.load(path)


def _header_params(name):
    """The parameter types of `name` as include/rbhip.h declares it."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rbhip.h")).read(), flags=re.S)
    m = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", src)
    assert m, name
    types = []
    for p in m.group(1).split(","):
        p = " ".join(p.split())
        t, star = re.match(r"(.*?)(\*?)\s*\w+$", p).groups()
        types.append((t.strip() + (" *" if star else "")).strip())
    return types


def test_entry_points_are_exported_with_the_headers_argument_lists(lib):
    from rbhip import _lib
    path = os.path.join(PKG, "rbhip", "librbhip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert not [f for f in FUNCS if f not in exported]
    assert b"0.4" in lib.rb_version()                      # additive: the version string stays
    want = {
        "rb_query_contacts": ["rb_world *", "int64_t", "int64_t", "int32_t", "int32_t *", "int32_t *", "int32_t *",
                              "double *", "double *", "double *", "int64_t *"],
        "rb_query_contacts_dev": ["rb_world *", "int64_t", "int64_t", "int32_t", "int32_t *", "int32_t *", "int32_t *",
                                  "void *", "void *", "void *", "int32_t"],
    }
    for f in FUNCS:
        params = _header_params(f)
        assert params == want[f], (f, params)
        res, args = _lib.SIGNATURES[f]
        assert res is C.c_int and args == [CTYPES[t] for t in params], f
        assert getattr(lib, f).argtypes == args


def test_null_world_and_python_surface(lib):
    import rbhip
    a = np.zeros(64, np.int32)
    p = a.ctypes.data_as(C.c_void_p)
    assert lib.rb_query_contacts(None, 0, 1, 0, p, None, None, None, None, None, None) == EINVAL
    assert b"null world" in lib.rb_last_error()
    assert lib.rb_query_contacts_dev(None, 0, 1, 0, p, None, None, None, None, None, 0) == EINVAL
    assert b"null world" in lib.rb_last_error()
    for m in ("query_contacts", "query_contacts_device", "contacts"):
        assert callable(getattr(rbhip.World, m)), m
    assert rbhip.WorldContacts is rbhip.world.WorldContacts
    fields = ("max_records", "counts", "partner", "kind", "dist", "pos", "frame", "truncated")
    wc = rbhip.WorldContacts(*range(8))
    bc = rbhip.BatchContacts(*range(8))
    for f in fields:
        assert getattr(wc, f) == getattr(bc, f), f


def _dense(counts, R, geometry=True, seed=0):
    """Hand-made dense arrays: record s of body k carries the values (k, s)."""
    import rbhip
    rng = np.random.default_rng(seed)
    n = len(counts)
    cnt = np.asarray(counts, np.int32).reshape(1, n)
    k, s = np.meshgrid(np.arange(n), np.arange(R), indexing="ij")
    used = s < np.clip(cnt.reshape(-1, 1), 0, R)
    partner = np.where(used, 100 * k + s, 0).astype(np.int32).reshape(1, n, R)
    kind = np.where(used, 16, -1).astype(np.int32).reshape(1, n, R)
    dist = np.where(used, -(k + s / 16.0), 0.0).reshape(1, n, R)
    pos = np.where(used[..., None], rng.normal(size=(n, R, 3)), 0.0).reshape(1, n, R, 3)
    frame = np.where(used[..., None], rng.normal(size=(n, R, 3)), 0.0).reshape(1, n, R, 3)
    trunc = int((cnt > R).sum())
    return rbhip.WorldContacts(R, cnt, partner, kind, dist, pos if geometry else None, frame if geometry else None, trunc)


def test_to_csr_shapes_truncated_rows_and_rows_without_a_list():
    counts = [0, 2, 5, -2, 3, 1, -2, 4]                    # 5 and 4 exceed R = 3; two bodies have no list
    R = 3
    con = _dense(counts, R)
    assert con.counts.shape == (1, 8) and con.partner.shape == (1, 8, R) and con.pos.shape == (1, 8, R, 3)
    assert con.truncated == 2
    cnt, par, kin, dis, pos, frm = con.to_csr()
    kept = np.clip(counts, 0, R)
    total = int(kept.sum())
    assert cnt.shape == (8,) and cnt.dtype == np.int32 and cnt.tolist() == counts     # counts stay as returned
    assert par.shape == kin.shape == dis.shape == (total,) and pos.shape == frm.shape == (total, 3)
    at = 0
    for k, c in enumerate(kept):
        for s in range(c):
            assert par[at] == 100 * k + s and kin[at] == 16 and dis[at] == -(k + s / 16.0)
            assert np.array_equal(pos[at], con.pos[0, k, s]) and np.array_equal(frm[at], con.frame[0, k, s])
            at += 1
    assert at == total and (kin >= 0).all()                # no unused slot is listed
    # the result is a copy: the query's arrays stay as they were
    cnt[0] = 9
    assert con.counts[0, 0] == 0


def test_to_csr_without_geometry_and_counts_only():
    import contact_geometry as cg
    import rbhip
    con = _dense([1, 0, 2], 4, geometry=False)
    cnt, par, kin, dis, pos, frm = con.to_csr()
    assert pos is None and frm is None and par.tolist() == [0, 200, 201] and cnt.tolist() == [1, 0, 2]
    # nothing truncated: the shape dense_lists takes unchanged, and the same lists
    full = _dense([1, 0, 2], 4)
    got = full.to_csr()
    want = cg.dense_lists(full)
    assert len(got) == len(want) == 6
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    only = rbhip.WorldContacts(0, np.array([[3, -2, 0]], np.int32), None, None, None, None, None, 1)
    cnt, *rest = only.to_csr()
    assert cnt.tolist() == [3, -2, 0] and rest == [None] * 5


def test_new_kernels_are_listed_without_scratch():
    out = subprocess.run(["make", "-s", "-C", os.path.join(PKG, "csrc"), "resource-usage"],
                         capture_output=True, text=True, check=True).stdout
    got = {}
    for m in re.finditer(r"Function Name: (\S*?\d+(world_contacts\w*?_kernel)I\S*)\s+(?:.*\n)*?.*ScratchSize \[bytes/lane\]: (\d+)", out):
        got.setdefault(m.group(2), []).append((m.group(1), int(m.group(3))))
    assert set(got) == KERNELS, sorted(got)
    for kern, inst in got.items():
        assert len(inst) == 2, (kern, inst)                # fp64 and fp32
        assert not [n for n, scratch in inst if scratch], kern
