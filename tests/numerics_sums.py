"""Shared by tests/golden/make_numerics_sums.py, tests/test_numerics_cpu.py and tests/test_hip_numerics.py: builds and runs
tests/numerics_sums_host.c (the CPU oracle's side of the exhaustive sweep of the numerics spec's scalar functions) and reads what it prints.
TEST INFRASTRUCTURE (CPU only)."""
from __future__ import annotations

import hashlib
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ORACLE_DIR = os.path.join(ROOT, "oracle")
FIXTURE = os.path.join(HERE, "golden", "numerics_sums.npz")
CHUNK_BITS = 20
CHUNK = 1 << CHUNK_BITS
NCHUNKS = 1 << (32 - CHUNK_BITS)
RECIP_LO, RECIP_HI = 0x40000000, 0x41100000                       # 2.0f, 9.0f
RECIP_CHUNK0 = RECIP_LO >> CHUNK_BITS
RECIP_NCHUNKS = (RECIP_HI >> CHUNK_BITS) - RECIP_CHUNK0 + 1         # 18: the last one holds 9.0f alone
# the floats the guard always recomputes: the chunks that hold them, and those chunks' left neighbours
LANDMARKS = (0x00000000, 0x3F800000, 0x40E00000, 0x7F800000, 0x7FC00000, 0x80000000, 0xC0E00000, 0xFF800000)
# the oracle's flags that bear on floating point (oracle/Makefile), for the host program's own division
HOST_CFLAGS = ["-O2", "-std=c11", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-Wall", "-Wextra"]


def guard_chunks():
    """The fixed subset: 16 chunks of a seeded draw, the landmark chunks and their left neighbours (modulo 4096), sorted."""
    draw = np.random.default_rng(20).choice(NCHUNKS, size=16, replace=False)
    cs = {int(c) for c in draw}
    for u in LANDMARKS:
        c = u >> CHUNK_BITS
        cs |= {c, (c - 1) % NCHUNKS}
    return sorted(cs)


def oracle_sha256():
    """SHA-256 of what decides the oracle's erfc_spec bits: its source, its header and the Makefile with the compiler flags."""
    h = hashlib.sha256()
    for name in ("llicti_oracle.c", "llicti_oracle.h", "Makefile"):
        with open(os.path.join(ORACLE_DIR, name), "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def build_host(out_dir):
    """gcc tests/numerics_sums_host.c against oracle/liboracle.so -> the executable's path (in out_dir)."""
    from oracle import oracle as orc
    orc.build()
    exe = os.path.join(str(out_dir), "numerics_sums_host")
    subprocess.check_call([os.environ.get("CC", "gcc")] + HOST_CFLAGS + ["-o", exe, os.path.join(HERE, "numerics_sums_host.c"),
                           "-L", ORACLE_DIR, "-loracle", "-Wl,-rpath," + ORACLE_DIR, "-lm"])
    return exe


def _env():
    env = dict(os.environ)
    env.setdefault("OMP_NUM_THREADS", "8")         # the program takes its thread count from here, never from the CPU count
    return env


def budget_args():
    import ref64
    return ["--budget", float(ref64.ERFC_REL).hex(), float(ref64.ERFC_TAIL).hex()]


def run_host(exe, mode_args, timeout=1200):
    """Run `all` or `chunks ...` with ref64's budget -> dict of arrays, one entry per chunk in the order printed:
    chunk, s1, s2 (uint64), min, max (uint32), rel, abs, ratio (float64) and their arguments' bits (uint32); recip: {chunk: (s1, s2)}."""
    r = subprocess.run([exe] + budget_args() + list(mode_args), capture_output=True, text=True, timeout=timeout, env=_env())
    assert r.returncode == 0, (r.returncode, r.stderr[-800:])
    E, recip = [], {}
    for line in r.stdout.splitlines():
        t = line.split()
        if t[0] == "E":
            E.append((int(t[1]), int(t[2], 16), int(t[3], 16), int(t[4], 16), int(t[5], 16), float.fromhex(t[6]), int(t[7], 16),
                      float.fromhex(t[8]), int(t[9], 16), float.fromhex(t[10]), int(t[11], 16)))
        elif t[0] == "R":
            recip[int(t[1])] = (int(t[2], 16), int(t[3], 16))
    cols = list(zip(*E))
    names = ("chunk", "s1", "s2", "min", "max", "rel", "rel_arg", "abs", "abs_arg", "ratio", "ratio_arg")
    types = (np.int64, np.uint64, np.uint64, np.uint32, np.uint32, np.float64, np.uint32, np.float64, np.uint32, np.float64, np.uint32)
    out = {n: np.array(c, dtype=t) for n, c, t in zip(names, cols, types)}
    out["recip"] = recip
    return out


def host_dump(exe, chunk, path):
    """The 2^20 output words of the oracle's erfc_spec over one chunk."""
    r = subprocess.run([exe, "dump", str(int(chunk)), str(path)], capture_output=True, text=True, timeout=120, env=_env())
    assert r.returncode == 0, (r.returncode, r.stderr[-800:])
    w = np.fromfile(str(path), dtype="<u4")
    assert w.size == CHUNK
    return w


def bits_to_float(u):
    return float(np.array([u], dtype=np.uint32).view(np.float32)[0])
