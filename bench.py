#!/usr/bin/env python3
"""Benchmark of the hot path: the miner's min-hash nonce scan on MI355X.

Contract (driver): ``python bench.py --gpus N --steps K --warmup W``; for N>1
it is launched by torch.distributed.run, one rank per GPU.  Rank 0 prints ONE
JSON line.

Workload (BASELINE.json configs[1]): message "bradfitz" (8 B, one SHA-256
tail block), 2^32 nonces per GPU.  One "step" = every rank scans its own
contiguous 2^32-nonce shard ([rank*2^32, (rank+1)*2^32)) on its GPU through
the C ABI (hm_scan), then ONE all-gather of the 16-byte (hash, nonce)
candidates (RCCL over xGMI for N>1) and a lexicographic min -- the exchange
step of the north star.  Per-GPU work is fixed as N grows: weak scaling.

value = nonces scanned by all ranks / time, in GH/s.  Inputs live on the GPU
(the only host input is the 8-byte message); the timed region covers the
whole hm_scan call (planning, all launches, the 16-B readback) and the merge.
`ranks` reports each rank's own time and GPU busy time (spread across GPUs).

A plain run does only that: it sets up, runs W untimed and K timed steps,
writes the last step's answers if --dump-outputs DIR is given (result.npy,
ranks.npy: see dump_outputs) and prints the line -- value, ms_per_step, the
per-rank timings and answers, the build identity.  Everything below is
measured or checked only with --full; the line's fields for it are null or
absent otherwise.

Secondary workloads of a --full run, under `workloads`: cfg3 (BASELINE
configs[2], the 120-B message on the same weak shards, 5 steps) and cfg4
(configs[3]: [0, 2^40) split over the N ranks by hm_partition -- strong
scaling, the configuration of the >= 7.5x target -- 1 step), each checked
against its oracle fixture.

roofline: INT32 VALU, SURVEY §8(d): algorithmic work = 1552 lane-ops per
SHA-256 compression x C compressions per nonce; achieved = that work in the
dominant scan launch / its HIP-event duration (measured live, on the stream
the kernel runs on); peak = 256 CU x 4 SIMD x 32 lanes x 2.4 GHz.
`frac_rounds` prices instead the rounds and schedule words the kernel's
formulation executes per nonce (rounds_ops_per_nonce).
Per-rank self-check: every workload's `ranks` carries each rank's own 16-B
answer, its device (ordinal, PCI address) and kernel GH/s, and `match` of
that answer against the fixture pieces tiling the rank's shard
(tests/golden/full_size.json); `all_ranks_match` sums them up.  Any mismatch
exits 1 after the line is printed.  `build_id` / `build_matches_tree` tie the
measured library to the sources beside this file.
single_process (multi-GPU runs): configs[3] once more through ONE process
driving every GPU (SURVEY §8(e)'s process model), after every timed region:
two fresh child processes with hard timeouts, one merging the 16-B shard
results on the host, one with the in-library RCCL all-gather; a child's
hang or abort is an entry of the line, never the loss of it.
cpu_baseline: the reference miner fleet restated on the host -- one thread
per core of this process's CPU share (<= 16), each a sequential miner over
its own chunk, running the C restatement of the reference loop
(oracle/hm_oracle.c: format + SHA-256 from the IV per nonce, strict <) on a
bounded sample of the same message; one miner alone is reported beside it.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PER_GPU = 1 << 32
MAXU64 = (1 << 64) - 1


def long120() -> bytes:
    """BASELINE configs[2] message: random.Random(440), 120 chars 0x21..0x7e."""
    import random
    rng = random.Random(440)
    return bytes(rng.choice(range(0x21, 0x7F)) for _ in range(120))


WORKLOADS = {
    # name: (message, description)
    "cfg2": (b"bradfitz", "cfg2: msg 'bradfitz' (8 B, C=1), 2^32 nonces per GPU "
                          "[rank*2^32, (rank+1)*2^32), all-gather of 16-B candidates"),
    "cfg3": (None, "cfg3: 120-B msg (random.Random(440)), C=2 (1 host-midstate block + 2 tail "
                   "blocks), 2^32 nonces per GPU, all-gather of 16-B candidates"),
    # strong scaling: the whole [0, 2^40) split over the N ranks
    "cfg4": (b"bradfitz", "cfg4: msg 'bradfitz', [0, 2^40) split contiguously over N GPUs "
                          "(strong scaling), all-gather of 16-B candidates"),
}


def fixture_check(msg: bytes, lo: int, hi: int, res):
    """Compare a whole-job answer with the committed oracle fixture of the
    same (message, range), if there is one: tests/golden/large.json (configs
    [1]/[2] over [0, 2^32)) and full_size.json (configs[3] over [0, 2^40),
    and the weak-scaling jobs [0, N*2^32) of configs[1]/[2] for N <= 8).
    Data only -- nothing under oracle/ is run here."""
    gold = os.path.join(ROOT, "tests", "golden")
    found = []
    try:
        with open(os.path.join(gold, "large.json")) as f:
            for c in json.load(f):
                found.append(("tests/golden/large.json", c))
        with open(os.path.join(gold, "full_size.json")) as f:
            full = json.load(f)
        c4 = full.get("cfg4")
        if c4:
            found.append(("tests/golden/full_size.json", dict(c4, **c4["whole"])))
        for w in full.get("weak", []):  # [0, N*2^32): the first N pieces
            for n in range(1, len(w["pieces"]) + 1):
                best = min((int(p["hash"]), int(p["nonce"])) for p in w["pieces"][:n])
                found.append(("tests/golden/full_size.json",
                              {"msg_hex": w["msg_hex"], "lo": "0", "hi": str((n << 32) - 1),
                               "hash": str(best[0]), "nonce": str(best[1])}))
    except (OSError, ValueError):
        return None
    for path, c in found:
        if bytes.fromhex(c["msg_hex"]) == msg and (int(c["lo"]), int(c["hi"])) == (lo, hi):
            exp = (int(c["hash"]), int(c["nonce"]))
            return {"fixture": path, "expected": {"hash": exp[0], "nonce": exp[1]},
                    "match": tuple(res) == exp}
    return None


def _fixture_pieces(msg: bytes):
    """Every list of contiguous oracle pieces the committed fixtures hold for
    msg: full_size.json's weak pieces (configs[1]/[2]: [r*2^32, (r+1)*2^32)
    for r < 8) and its cfg4 pieces (configs[3]: [0, 2^40) in 2^34-nonce
    pieces, cut at every hm_partition boundary for 1/2/4/8 shards)."""
    try:
        with open(os.path.join(ROOT, "tests", "golden", "full_size.json")) as f:
            full = json.load(f)
    except (OSError, ValueError):
        return []
    lists = [w["pieces"] for w in full.get("weak", []) if bytes.fromhex(w["msg_hex"]) == msg]
    c4 = full.get("cfg4")
    if c4 and bytes.fromhex(c4["msg_hex"]) == msg:
        lists.append(c4["pieces"])
    return lists


def shard_check(msg: bytes, lo, hi, res):
    """One rank's own 16-B answer against the oracle pieces that make up its
    shard [lo, hi] exactly (None when no fixture covers it).  An empty shard
    (lo None) must answer the scan's seed (2^64-1, 0)."""
    if lo is None:
        return {"fixture": None, "expected": {"hash": MAXU64, "nonce": 0},
                "match": tuple(res) == (MAXU64, 0)}
    for pieces in _fixture_pieces(msg):
        inside = sorted((p for p in pieces if int(p["lo"]) >= lo and int(p["hi"]) <= hi),
                        key=lambda p: int(p["lo"]))
        if not inside or int(inside[0]["lo"]) != lo or int(inside[-1]["hi"]) != hi:
            continue
        if any(int(b["lo"]) != int(a["hi"]) + 1 for a, b in zip(inside, inside[1:])):
            continue
        exp = min((int(p["hash"]), int(p["nonce"])) for p in inside)
        return {"fixture": "tests/golden/full_size.json",
                "expected": {"hash": exp[0], "nonce": exp[1]}, "match": tuple(res) == exp}
    return None


SP_TIMEOUT_S = 180  # per single-process child (configs[3] on one GPU opened twice: ~60 s)
# HIP streams per GPU of every hipminer context this bench opens (ranks and
# single-process children; HM_OPT_STREAMS, made on first use since ABI 1.8):
# each stream holds a hardware queue until its process exits, and the GPU
# time-slices once the processes on it hold more than ~20 queues.
# 2 = the dominant kernel's stream + one tail-filling stream.
BENCH_STREAMS = int(os.environ.get("HM_BENCH_STREAMS", "2") or 2)
KFD_PROC = "/sys/class/kfd/kfd/proc"
KFD_TOPOLOGY = "/sys/class/kfd/kfd/topology/nodes"


def kfd_gpu_pci():
    """KFD gpu_id -> PCI address ("dddd:bb:dd.f") from KFD's topology (sysfs;
    no GPU call).  Empty when KFD is not visible."""
    out = {}
    try:
        nodes = os.listdir(KFD_TOPOLOGY)
    except OSError:
        return out
    for n in nodes:
        try:
            with open(os.path.join(KFD_TOPOLOGY, n, "gpu_id")) as f:
                gid = f.read().strip()
            props = {}
            with open(os.path.join(KFD_TOPOLOGY, n, "properties")) as f:
                for line in f:
                    k, _, v = line.partition(" ")
                    props[k] = v.strip()
        except OSError:
            continue
        if gid in ("", "0") or "location_id" not in props:
            continue
        loc, dom = int(props["location_id"]), int(props.get("domain", "0"))
        out[gid] = f"{dom:04x}:{loc >> 8:02x}:{(loc >> 3) & 0x1f:02x}.{loc & 7}"
    return out


def kfd_queues():
    """User-mode (hardware) queues per GPU right now, over every process KFD
    knows (/sys/class/kfd/kfd/proc/<pid>/queues/<qid>/gpuid): {gpu_id:
    {"queues": q, "processes": p}}, or {"error": ...} when KFD is not
    readable.  Sysfs only, so it can run beside a GPU job."""
    try:
        pids = os.listdir(KFD_PROC)
    except OSError as e:
        return {"error": f"{KFD_PROC}: {type(e).__name__}"}
    out = {}
    for pid in pids:
        qdir = os.path.join(KFD_PROC, pid, "queues")
        try:
            qids = os.listdir(qdir)
        except OSError:
            continue
        seen = set()
        for q in qids:
            try:
                with open(os.path.join(qdir, q, "gpuid")) as f:
                    gid = f.read().strip()
            except OSError:
                continue
            e = out.setdefault(gid, {"queues": 0, "processes": 0})
            e["queues"] += 1
            if gid not in seen:
                seen.add(gid)
                e["processes"] += 1
    return out


class QueueSampler:
    """Samples kfd_queues() on a thread while a single-process child runs and
    keeps each GPU's maximum: the queues and processes the GPUs actually
    carried (the line recorded only a modelled process count)."""

    def __init__(self, period_s: float = 0.25, pcis=None):
        import threading
        self.period_s, self.max, self.error, self.samples = period_s, {}, None, 0
        self.pcis = set(pcis) if pcis else None  # report only these GPUs (PCI addresses)
        self._stop = threading.Event()
        self._t = threading.Thread(target=self._run, daemon=True)

    def _run(self):
        while True:
            q = kfd_queues()
            if "error" in q:
                self.error = q["error"]
            else:
                self.samples += 1
                for g, e in q.items():
                    m = self.max.setdefault(g, {"queues": 0, "processes": 0})
                    m["queues"] = max(m["queues"], e["queues"])
                    m["processes"] = max(m["processes"], e["processes"])
            if self._stop.wait(self.period_s):
                return

    def __enter__(self):
        self._t.start()
        return self

    def __exit__(self, *exc):
        self._stop.set()
        self._t.join(timeout=5)

    def result(self) -> dict:
        if self.error and not self.samples:
            return {"error": self.error}
        per_gpu = by_pci(self.max, self.pcis)
        return {"samples": self.samples, "period_s": self.period_s, **per_gpu,
                "max_queues_any_gpu": max((v["queues"] for v in per_gpu["max"].values()),
                                          default=0)}


def by_pci(counts: dict, pcis=None) -> dict:
    """{gpu_id: counts} keyed by PCI address instead; with `pcis`, only those
    GPUs (the job's), the others only counted: KFD lists every process on
    the host, other jobs' GPUs included."""
    pci = kfd_gpu_pci()
    named = {pci.get(g, f"gpu_id {g}"): v for g, v in sorted(counts.items())}
    if pcis is None:
        return {"max": named}
    return {"max": {k: v for k, v in named.items() if k in pcis},
            "other_gpus": sum(1 for k in named if k not in pcis)}


def single_process_cfg4(devices, rccl: bool):
    """configs[3] ([0, 2^40) of "bradfitz") through ONE process driving every
    device in `devices` -- SURVEY §8(e)'s own process model (one hm_open over
    the device list, hm_partition shards, 16-B results merged on the host, or
    with the in-library RCCL all-gather when `rccl`).  Timed once after a
    small untimed warm-up scan; checked against full_size.json's whole-range
    answer.  Runs in a child process (run_single_process).  Never raises: a
    failure is reported in the returned dict."""
    from distributed_bitcoinminer_amd import _lib
    m, hi = WORKLOADS["cfg4"][0], (1 << 40) - 1
    merge_req = "rccl" if rccl else "host"
    try:
        with _lib.Context(devices) as c:
            c.set_option(_lib.HM_OPT_STREAMS, BENCH_STREAMS)
            if rccl:
                c.set_option(_lib.HM_OPT_MERGE_RCCL, 1)
            c.scan(m, 0, 10**9)  # module load, first launches, RCCL communicator
            t = time.perf_counter()
            res = c.scan(m, 0, hi)
            el = time.perf_counter() - t
            st = c.stats()
    except Exception as e:  # reported, never fatal to the bench line
        return {"devices": list(devices), "merge_requested": merge_req,
                "error": f"{type(e).__name__}: {e}"}
    merge = {_lib.HM_MERGE_NONE: "none", _lib.HM_MERGE_HOST: "host",
             _lib.HM_MERGE_RCCL: "RCCL all-gather"}.get(st["merge"], str(st["merge"]))
    return {"devices": list(devices), "merge_requested": merge_req, "merge": merge,
            "value": round((hi + 1) / el / 1e9, 3), "unit": "GH/s", "wall_ms": round(el * 1e3, 3),
            # kernel_ms sums the devices' busy time: nonces / it = the mean
            # per-device kernel rate
            "kernel_GHs_per_device": round((hi + 1) / st["kernel_ms"] / 1e6, 3)
            if st["kernel_ms"] > 0 else None,
            "enqueue_ms": round(st["enqueue_ms"], 3), "mid_call_syncs": st["mid_call_syncs"],
            "streams_per_gpu": BENCH_STREAMS,
            "result": {"hash": res[0], "nonce": res[1]},
            "result_vs_oracle": fixture_check(m, 0, hi, res)}


def _sp_child_main(merge: str, devices: str) -> None:
    """Entry of a single-process child (`bench.py --sp-child host|rccl
    --sp-devices 0,1,...`): one JSON object on stdout, exit status 0 unless
    the interpreter itself dies.  No torch import: the child holds only its
    hipminer context on the GPUs."""
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)  # RCCL's banner and the like go to stderr
    out = single_process_cfg4([int(x) for x in devices.split(",") if x != ""], merge == "rccl")
    os.write(json_fd, (json.dumps(out) + "\n").encode())


def _run_child(cmd, timeout: float) -> dict:
    """Run one single-process child in its own session; its last stdout line
    is its JSON result.  A timeout kills the child's process group (by the
    PID this function started), an abnormal exit or unreadable output is an
    `error` entry: never an exception."""
    import signal
    import subprocess
    t0 = time.perf_counter()
    try:
        p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                             start_new_session=True, cwd=ROOT)
    except OSError as e:
        return {"error": f"could not start: {e}"}
    try:
        out, err = p.communicate(timeout=timeout)
    except subprocess.TimeoutExpired:
        try:
            os.killpg(p.pid, signal.SIGKILL)
        except OSError:
            pass
        try:
            p.communicate(timeout=15)
        except subprocess.TimeoutExpired:
            pass
        return {"timeout": timeout, "error": f"no result within {timeout} s (child killed)"}
    elapsed = round(time.perf_counter() - t0, 3)
    lines = [l for l in out.splitlines() if l.startswith("{")]
    if p.returncode != 0 or not lines:
        return {"error": f"child exit status {p.returncode}", "child_s": elapsed,
                "stderr_tail": err[-600:]}
    try:
        res = json.loads(lines[-1])
    except ValueError:
        return {"error": "unreadable child output", "child_s": elapsed, "stdout_tail": out[-600:]}
    res["child_s"] = elapsed
    return res


def run_single_process(devices, rank_gpus, timeout: float = SP_TIMEOUT_S, child_cmd=None,
                       pcis=None) -> dict:
    """configs[3] through SURVEY §8(e)'s single-process model, measured by
    rank 0 after every timed region of a multi-GPU line: one hipminer context
    over every GPU in `devices`, twice, each in a FRESH CHILD PROCESS with a
    hard timeout -- `host` merges the 16-B shard results on the host, `rccl`
    with the in-library RCCL all-gather (ncclCommInitAll over the distinct
    ordinals of `devices`, grouped ncclAllGather, device-side fold).  A hang,
    abort or wrong answer in a child becomes an entry of this dict; the bench
    line is printed either way.  `processes_per_gpu` counts the processes
    that hold a context on each GPU while a child runs: every rank's own
    process (its torch context and communicator on its GPU, rank_gpus[r])
    plus the child; `queues_per_gpu` per child the hardware queues KFD shows on
    each of the job's GPUs (`pcis`, PCI addresses) while it runs.
    child_cmd(merge, devices) -> argv is a test hook."""
    rccl_devs = sorted(set(devices))
    if child_cmd is None:
        def child_cmd(merge, devs):
            return [sys.executable, os.path.abspath(__file__), "--sp-child", merge,
                    "--sp-devices", ",".join(str(d) for d in devs)]
    per_gpu = {}
    for d in devices:
        per_gpu[d] = 1  # the child
    for g in rank_gpus:  # each rank's own process on its GPU
        if g in per_gpu:
            per_gpu[g] += 1
    out = {"workload": "cfg4 in one process: hm_open over every GPU, [0, 2^40) as "
                       "hm_partition shards, 16-B results merged (SURVEY 8(e)); one fresh "
                       "child process per merge, each with a hard timeout",
           "devices": list(devices), "timeout_s": timeout,
           "processes_per_gpu": {str(k): v for k, v in sorted(per_gpu.items())}}
    for merge, devs in (("host", list(devices)), ("rccl", rccl_devs)):
        # the queues every process on each GPU holds while this child runs
        # (KFD sysfs, sampled; keyed by PCI address)
        with QueueSampler(pcis=pcis) as qs:
            res = _run_child(child_cmd(merge, devs), timeout)
        res.setdefault("devices", devs)
        res["queues_per_gpu"] = qs.result()
        out[merge] = res
    return out


def wrong_answers(line) -> list:
    """Checks of a bench line whose answer differs from its oracle fixture:
    the whole-job answers, the per-rank answers and the single-process
    children's answers.  A child's error or timeout is reported in the line
    but is not a wrong answer (the run's exit status stays 0)."""
    secondary = line.get("workloads", {})
    checks = [line["result_vs_oracle"], *(w["result_vs_oracle"] for w in secondary.values())]
    sp = line.get("single_process") or {}
    checks += [(sp.get(m) or {}).get("result_vs_oracle") for m in ("host", "rccl")]
    wrong = [c for c in checks if c is not None and c["match"] is False]
    wrong += [n for n, rk in [("primary", line["ranks"])] +
              [(k, w["ranks"]) for k, w in secondary.items()] if all_match(rk) is False]
    return wrong


def all_match(ranks):
    """True when every rank's answer equals its fixture piece, False when any
    differs, None when some rank has no fixture (and none differs)."""
    m = ranks["match"]
    if any(x is False for x in m):
        return False
    return True if all(x is True for x in m) else None


def code_object_sha16():
    """sha256 (16 hex) of the scan kernels' code object embedded in the
    libhipminer.so this process loaded (the bytes hipModuleLoadData gets), so a
    PMC summary is matched to the build that actually runs; None if the
    library cannot be loaded."""
    try:
        from distributed_bitcoinminer_amd import _lib
        return _lib.code_object_sha16()
    except Exception:
        return None


def profiled(kernel: str):
    """PMC summary of `kernel` from the newest committed profile
    (profiles/rNN/pmc_summary.json, written by tools/summarize_profile.py):
    HBM bytes per nonce, the effective clock and the measured VALU
    instructions per nonce (SQ_INSTS_VALU per 64-nonce wave iteration), with
    the file they came from.  Only a summary recorded for THIS build's code
    object (its `code_object_sha16`) counts: a stale one gives Nones."""
    import glob
    sha = code_object_sha16()
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", "pmc_summary.json")),
                       reverse=True):
        with open(path) as f:
            summ = json.load(f)
        if kernel in summ:
            k = summ[kernel]
            if sha is None or k.get("code_object_sha16") != sha:
                return None, None, None, None
            # HBM bytes per nonce of the profiled workload (its launches may
            # be sized differently from the bench's)
            per_nonce = k["hbm_bytes_per_launch"] * k["launches"] / k["nonces"]
            return per_nonce, k["f_eff_ghz_largest_dispatch"], \
                k.get("valu_insts_per_wave_iteration_64_nonces"), os.path.relpath(path, ROOT)
    return None, None, None, None


OPS_PER_COMPRESSION = 1552
PEAK_TOPS = 256 * 4 * 32 * 2.4e9 / 1e12   # 78.64 T INT32 lane-ops/s
CPU_SAMPLE = 50_000_000              # nonces for the 1-thread CPU baseline (~12 s on the GPU box host)
CPU_FLEET_PER_THREAD = 40_000_000    # nonces per thread of the fleet sample (~9 s)
CPU_FAST_PER_THREAD = 60_000_000     # nonces per thread of the optimised CPU sample (~5 s)


def _cpu_share() -> int:
    """Host threads this process may use: its affinity set, capped at the GPU
    box's per-GPU share (16; OMP_NUM_THREADS is set to it there)."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    return max(1, min(n, int(os.environ.get("OMP_NUM_THREADS", "16") or 16), 16))


def cpu_baseline(msg: bytes, name: str):
    """The reference miner fleet restated on the host: one
    sequential miner per core on disjoint equal chunks (oracle/hm_oracle.c:
    Sprintf-style format + SHA-256 from the IV per nonce, strict <), plus one
    miner alone."""
    import platform
    from oracle import oracle
    oracle.build()
    oracle.c_scan(msg, 0, 100_000, threads=1)  # warm
    scale = 1 if len(msg) + 21 <= 55 else 3  # 1 vs 3 compressions per nonce
    n1 = CPU_SAMPLE // scale
    t = time.perf_counter()
    oracle.c_scan(msg, 0, n1 - 1, threads=1)
    d1 = time.perf_counter() - t
    cores = _cpu_share()
    nN = CPU_FLEET_PER_THREAD // scale * cores
    t = time.perf_counter()
    oracle.c_scan(msg, 0, nN - 1, threads=cores)
    dN = time.perf_counter() - t
    cpu = next((l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo")
                if l.startswith("model name")), platform.processor() or "?")
    # SURVEY §8(d)'s optional "optimised CPU" line: the SHA-extension oracle
    # (midstate of the constant blocks, digits incremented in place, x86 SHA
    # instructions), same threads; not the reference's per-nonce work
    optimised = None
    if oracle.fast_available():
        nF = CPU_FAST_PER_THREAD // scale * cores
        t = time.perf_counter()
        oracle.fast_scan_sum(msg, 0, nF - 1, threads=cores)
        dF = time.perf_counter() - t
        optimised = {"value": nF / dF / 1e9, "unit": "GH/s", "cores": cores,
                     "sample": f"[0, {nF}) on {cores} threads of oracle/hm_oracle_fast.c "
                               f"(SHA extensions, midstate, in-place digits), {dF:.2f} s"}
    return {"value": nN / dN / 1e9, "unit": "GH/s", "cores": cores, "kind": "port",
            "sample": f"{name}: a fleet of {cores} CPU miners (one thread each, disjoint equal "
                      f"chunks of [0, {nN})) running oracle/hm_oracle.c, the C restatement of "
                      f"the reference loop (Sprintf-style format + SHA-256 from the IV per "
                      f"nonce, strict <); {dN:.2f} s on {cpu}",
            "single_miner": {"value": n1 / d1 / 1e9, "unit": "GH/s", "cores": 1,
                             "sample": f"[0, {n1}) on 1 thread, {d1:.2f} s"},
            "optimised": optimised}


ROUND_OPS = 16      # lane-ops per SHA-256 round
SCHED_OPS = 11      # ... per message-schedule word (64 x 16 + 48 x 11 = 1552)


def _sched_deps(varying):
    """Schedule words W16..W63 that depend on any message word in `varying`
    (W[t] = s1(W[t-2]) + W[t-7] + s0(W[t-15]) + W[t-16])."""
    dep = [i in varying for i in range(64)]
    for t in range(16, 64):
        dep[t] = dep[t - 2] or dep[t - 7] or dep[t - 15] or dep[t - 16]
    return {t for t in range(16, 64) if dep[t]}


def rounds_ops_per_nonce(seg, c_eff):
    """Lane-ops per nonce that the segment's kernel formulation executes,
    priced at SURVEY's 16 per round and 11 per schedule word, with the work
    it hoists out of the per-nonce loop amortised over the nonces it serves
    (DESIGN.md §5 "frac_rounds").

    tiled (hm_tiled_kernel<W1, S, T>): rounds 0..W1 run once per tens digit
      (10 nonces), round W1 then costs 2 adds per nonce (closed form), rounds
      W1+1..63 per nonce; schedule words that depend on the loop word W[W1]
      per nonce, those that depend on the straddled tens digit in W[W1-1] per
      10 nonces, the rest once per task (100 nonces); a constant trailer
      block is 64 table-driven rounds per nonce.
    chained: the final block's schedule is wave-uniform (the K+W table), so
      64 rounds per nonce, plus the per-lane block 0 (a full 1552) c_eff - 1
      times per nonce (counted exactly by the library), plus the table build
      (48 schedule words + 64 K adds per row, 10^f rows per segment).
    generic: 1552 per compression."""
    kind = seg["kind"]
    if kind == 2:  # tiled
        W1 = seg["W1"]
        loop = _sched_deps({W1})
        t1 = _sched_deps({W1 - 1}) - loop if seg["straddle"] else set()
        rest = 48 - len(loop) - len(t1)
        ops = (63 - W1) * ROUND_OPS + 2 + (W1 + 1) * ROUND_OPS / 10
        ops += len(loop) * SCHED_OPS + len(t1) * SCHED_OPS / 10 + rest * SCHED_OPS / 100
        if seg["trailer"]:
            ops += 64 * ROUND_OPS
        return ops, 0.0
    if kind == 3:  # chained; the table build is returned per segment
        ops = 64 * ROUND_OPS + OPS_PER_COMPRESSION * (c_eff - 1.0)
        return ops, 10 ** seg["f"] * (48 * SCHED_OPS + 64)
    return OPS_PER_COMPRESSION * max(1, c_eff), 0.0


def roofline(st, msg, lo, hi):
    """Roofline object of the dominant scan kernel of the last hm_scan (st =
    hm_stats).  achieved = ops per launch / average launch time (HIP events
    on the launch stream), with the ops priced per kernel kind (`pricing`):
      tiled ("1552 x C"): SURVEY §8(d)'s 1552 lane-ops per compression x the
        compressions per nonce the kernel runs (1, or 2 with a constant
        trailer block; dom_compressions_eff);
      chained ("rounds"): the rounds and schedule words the kernel's
        formulation executes (rounds_ops_per_nonce) -- its final block's
        schedule is a wave-uniform K+W table and block 0 is hoisted out of the
        loop, so pricing either at 1552 lane-ops would credit work the kernel
        never does (1552 x C_eff gave 0.97, 1552 x C 1.94).
    `frac_algorithmic_C` always prices SURVEY's fixed 1552*C with C counted
    before any hoisting (equal to `frac` for one-block tiled tails); for the
    chained kernel it exceeds 1 by construction (block 0 once per ~1000
    nonces).  `frac_rounds` is the rounds pricing for every kind."""
    from distributed_bitcoinminer_amd import _lib
    C = st["dom_compressions"]
    C_eff = st["dom_compressions_eff"] or C
    launches = max(1, st["dom_launches"])
    avg_ms = st["dom_kernel_ms"] / launches
    nonces_pl = st["dom_nonces"] / launches
    achieved = nonces_pl * OPS_PER_COMPRESSION * C_eff / (avg_ms * 1e-3) / 1e12
    achieved_alg = nonces_pl * OPS_PER_COMPRESSION * C / (avg_ms * 1e-3) / 1e12
    traffic_pn, f_eff, valu_pmc, traffic_src = profiled(st["dom_kernel"])
    traffic = round(traffic_pn * nonces_pl) if traffic_pn is not None else None
    # the dominant kernel's segments (one instantiation may serve several)
    segs = _lib.debug_plan(msg, lo, hi)
    dom_seg = max(segs, key=lambda s: s["hi"] - s["lo"])
    dom_segs = [s for s in segs if (s["kind"], s["W1"], s["straddle"], s["trailer"]) ==
                (dom_seg["kind"], dom_seg["W1"], dom_seg["straddle"], dom_seg["trailer"])]
    if dom_seg["kind"] == 3:
        dom_segs = [s for s in segs if s["kind"] == 3]
    rops, table = 0.0, 0.0
    for sg in dom_segs:
        o, t = rounds_ops_per_nonce(sg, C_eff)
        rops += o * (sg["hi"] - sg["lo"] + 1)
        table += t
    rops = (rops + table) / max(1, sum(s["hi"] - s["lo"] + 1 for s in dom_segs))
    achieved_rounds = nonces_pl * rops / (avg_ms * 1e-3) / 1e12
    # algorithmic HBM bytes of one dominant launch: its 128-B tile records
    # (10^V nonces each) + one 16-B candidate per wave of the grid; the
    # work queue adds one device-scope atomicAdd per 4 dequeued tasks (the
    # workgroup's LDS dispenser, scan_tasks.hpp kLdsBatch)
    tiles_pl = -(-int(nonces_pl) // 10 ** dom_seg["V"])
    algo_bytes = tiles_pl * 128 + st["dom_grid"] * 4 * 16
    tasks_pl = int(nonces_pl) // 6400 if dom_seg["kind"] == 2 else None  # tiled unit = 64 lanes x 100
    # tasks per queue atomic (api.cpp queue_shift): 16 for launches of >= 10^11 nonces
    queue_batch = 16 if nonces_pl >= 1e11 else 4
    chained = dom_seg["kind"] == 3
    if chained:  # priced by what the formulation executes (see docstring)
        achieved, ops_pn, pricing = achieved_rounds, rops, "rounds"
        note = (f"chained kernel: final-block schedule from a wave-uniform K+W table, block 0 "
                f"hoisted (once per {1 / max(C_eff - 1, 1e-9):.0f} nonces): frac prices the "
                f"executed rounds and schedule words; 1552 x C ({C}) would count "
                f"{OPS_PER_COMPRESSION * C - rops:.0f} ops per nonce the kernel never runs")
    else:
        ops_pn, pricing = OPS_PER_COMPRESSION * C_eff, "1552 x C"
        note = ("tiled kernel: SURVEY 8(d)'s 1552 lane-ops per compression x the "
                "compressions per nonce it runs")
    return {"bound": "valu", "achieved": round(achieved, 3),
            "peak": round(PEAK_TOPS, 3), "unit": "T int32 lane-ops/s",
            "frac": round(achieved / PEAK_TOPS, 4),
            "pricing": pricing, "pricing_note": note,
            "compressions_per_nonce": round(C_eff, 6),
            "frac_algorithmic_C": round(achieved_alg / PEAK_TOPS, 4),
            "compressions_per_nonce_algorithmic": C,
            "frac_rounds": round(achieved_rounds / PEAK_TOPS, 4),
            "ops_per_nonce_rounds": round(rops, 2),
            "traffic": traffic,
            "traffic_unit": "HBM bytes per launch (PMC FETCH_SIZE x2 + WRITE_SIZE)",
            "traffic_source": traffic_src,
            "algorithmic_bytes_per_launch": algo_bytes,
            "queue_units_per_launch": tasks_pl,
            "queue_atomics_per_launch": -(-tasks_pl // queue_batch) if tasks_pl is not None
            else None,
            "queue_tasks_per_atomic": queue_batch,
            "traffic_note": f"PMC traffic is the work queue's device-scope atomics "
                            f"(one per {queue_batch} dequeued tasks, executed memory-side), "
                            f"not re-reads (DESIGN.md §9)",
            "f_eff_ghz": f_eff,
            "frac_at_f_eff": round(achieved / (PEAK_TOPS * f_eff / 2.4), 4) if f_eff else None,
            "kernel": st["dom_kernel"],
            "launches_per_step": launches,
            "avg_launch_ms": round(avg_ms, 3),
            "nonces_per_launch": int(nonces_pl),
            "ops_per_nonce": round(ops_pn, 3),
            "valu_instr_per_nonce_pmc": round(valu_pmc, 1) if valu_pmc else None,
            # executed lane-ops (PMC VALU instructions x 64 lanes per 64
            # nonces) / peak: the issue-level fraction
            "executed_frac": round(valu_pmc * st["dom_nonces"]
                                   / (st["dom_kernel_ms"] * 1e-3) / 1e12
                                   / PEAK_TOPS, 4) if valu_pmc else None,
            "kernel_GHs": round(st["dom_nonces"] / (st["dom_kernel_ms"] * 1e-3) / 1e9, 3)}


def u64_words(pairs):
    """(hash, nonce) u64 pairs as a float64 array [n, 4]: hash >> 32, hash &
    0xffffffff, nonce >> 32, nonce & 0xffffffff.  float64 holds every 32-bit
    word exactly (a whole u64 it would round), so equal arrays mean equal
    answers."""
    import numpy as np
    m = 0xFFFFFFFF
    return np.array([[h >> 32, h & m, n >> 32, n & m] for h, n in pairs], dtype=np.float64)


def dump_outputs(path: str, res, answers) -> None:
    """--dump-outputs: what the last timed step returned, as float64 .npy
    files under `path` (made if missing; 32 bytes per rank and 32 for the
    merge, so nothing is sampled):
      result.npy  [4]     the step's merged (hash, nonce), as u64_words
      ranks.npy   [N, 4]  each rank's own hm_scan answer of that step
    The inputs are the fixed message and nonce ranges of the workload, so
    two builds run with the same arguments write comparable files."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "result.npy"), u64_words([res])[0])
    np.save(os.path.join(path, "ranks.npy"),
            u64_words([(a["hash"], a["nonce"]) for a in answers]))


def main():
    # stdout carries exactly one JSON line (rank 0): whatever the libraries
    # print (RCCL's version banner, gloo's connection notes) goes to stderr
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--secondary", default="cfg3,cfg4",
                    help="with --full: comma list of workloads timed after the primary cfg2 "
                         "run and reported under `workloads` (cfg3: weak, 5 steps; cfg4: "
                         "strong [0, 2^40), 1 step)")
    ap.add_argument("--no-secondary", action="store_true",
                    help="skip the secondary measurements of a --full cfg2 run")
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="cfg2")
    ap.add_argument("--full", action="store_true",
                    help="beside the timed steps: the oracle-fixture checks of every answer, "
                         "the roofline, the secondary workloads, the KFD queue counts, the "
                         "single-process children and the CPU baseline.  Without it the run "
                         "sets up, warms up, times --steps steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write what the last timed step returned "
                         "as DIR/<name>.npy (float64; see dump_outputs)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    msg, desc = WORKLOADS[args.workload]
    if msg is None:
        msg = long120()
    # Rehearsal on a 1-GPU box: HM_BENCH_BACKEND=gloo lets N ranks share GPU 0
    # (RCCL refuses two ranks on one device).  The driver's runs use nccl.
    backend = os.environ.get("HM_BENCH_BACKEND", "nccl")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")

    import numpy as np
    import torch
    from distributed_bitcoinminer_amd import _lib
    from distributed_bitcoinminer_amd.parallel import merge, shard_range

    gpu = local_rank if backend == "nccl" else 0
    dist = None
    # HM_BENCH_FORCE_DIST=1 runs the distributed path even at world size 1
    # (rehearses the RCCL all-gather on a 1-GPU box).
    use_dist = world > 1 or os.environ.get("HM_BENCH_FORCE_DIST") == "1"
    if use_dist:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(gpu)
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world,
                                    device_id=torch.device("cuda", gpu))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    ctx = _lib.Context([gpu])
    # the library this run measures, and whether it is this tree's build
    # (hm_build_id vs the digest of csrc/ and include/hipminer.h)
    from distributed_bitcoinminer_amd import build_id as bid
    build = {"build_id": _lib.build_id(), "build_matches_tree": _lib.build_id() == bid.tree_digest()}
    exit_code = 0
    # BENCH_STREAMS (HM_BENCH_STREAMS, default 2) streams per GPU; 1 =
    # strictly serial launches (kernel traces then attribute time without
    # cross-stream queue waits)
    ctx.set_option(_lib.HM_OPT_STREAMS, BENCH_STREAMS)
    dev = torch.device("cuda", gpu) if backend == "nccl" else torch.device("cpu")
    cdev = torch.device("cuda", gpu)
    cand = torch.empty(2, dtype=torch.int64, device=dev)
    gathered = torch.empty(2 * world, dtype=torch.int64, device=dev)

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize(cdev)

    def gather(vals, dtype):
        """All ranks' vectors (one all-gather, outside the timed region; the
        bench's only collectives besides the 16-B candidates)."""
        if dist is None:
            return [list(vals)]
        t = torch.tensor(vals, dtype=dtype, device=dev)
        out = torch.empty(world * len(vals), dtype=dtype, device=dev)
        dist.all_gather_into_tensor(out, t)
        return out.cpu().reshape(world, len(vals)).tolist()

    def gather_f64(vals):
        return gather(vals, torch.float64)

    # this rank's GPU, reported per rank so a wrong or slow shard names its device
    props = torch.cuda.get_device_properties(cdev)
    my_device = [gpu, props.pci_domain_id, props.pci_bus_id, props.pci_device_id]

    if dist is not None:
        # communicator set-up (RCCL connects its rings on the first
        # collective): one untimed all-gather of the candidate buffer, so a
        # run with --warmup 0 does not time connection set-up as scan work
        cand.zero_()
        dist.all_gather_into_tensor(gathered, cand)
        barrier()

    def measure(m, lo, hi, steps, warmup, shard_bounds):
        """W untimed + K timed steps of (this rank's hm_scan of [lo, hi],
        all-gather of the 16-B candidates, min).  Returns the max-over-ranks
        time, the merged result, rank 0's step times, this rank's hm_stats of
        the last scan and the per-rank timings (each rank's own time to its
        last result, before the closing barrier, and its summed scan-kernel
        busy time: DVFS or placement imbalance between GPUs shows there),
        with each rank's own answer, device and fixture match (shard_bounds(r)
        = rank r's inclusive shard, or (None, None) when empty)."""
        last_local = [None]

        def step():
            local = ctx.scan(m, lo, hi) if lo is not None else (MAXU64, 0)
            last_local[0] = local
            if dist is None:
                return local
            cand.copy_(torch.from_numpy(np.array(local, dtype=np.uint64).view(np.int64)))
            dist.all_gather_into_tensor(gathered, cand)  # 16 B per rank over RCCL
            arr = gathered.cpu().numpy().view(np.uint64).reshape(world, 2)
            return merge((int(a), int(b)) for a, b in arr)

        res = None
        for _ in range(warmup):
            res = step()
        barrier()
        t0 = time.perf_counter()
        step_ms, busy_ms = [], 0.0
        for _ in range(steps):
            ts = time.perf_counter()
            res = step()  # hm_scan returns after its 16-B readback: the step is complete
            step_ms.append((time.perf_counter() - ts) * 1e3)
            if lo is not None:
                busy_ms += ctx.stats()["kernel_ms"]
        torch.cuda.synchronize(cdev)
        local_ms = (time.perf_counter() - t0) * 1e3
        barrier()
        elapsed = time.perf_counter() - t0
        st = ctx.stats() if lo is not None else None
        kern_ghs = st["dom_nonces"] / (st["dom_kernel_ms"] * 1e-3) / 1e9 \
            if st and st["dom_kernel_ms"] > 0 else 0.0
        per_rank = gather_f64([local_ms, busy_ms, elapsed, kern_ghs])
        elapsed = max(r[2] for r in per_rank)
        loc = [round(r[0], 3) for r in per_rank]
        # per-rank self-check: each rank's own 16-B answer (u64 pair carried
        # as int64 bits), its device, and its answer against the oracle pieces
        # of its shard, so a wrong shard names its rank and GPU
        own = np.array(last_local[0], dtype=np.uint64).view(np.int64).tolist()
        ids = gather(own + [-1 if lo is None else 0] + my_device, torch.int64)
        answers, devices, match = [], [], []
        for r, row in enumerate(ids):
            a = tuple(int(x) for x in np.array(row[:2], dtype=np.int64).view(np.uint64))
            answers.append({"hash": a[0], "nonce": a[1]})
            devices.append({"ordinal": row[3],
                            "pci_bus_id": f"{row[4]:04x}:{row[5]:02x}:{row[6]:02x}.0"})
            chk = shard_check(m, *shard_bounds(r), a) if args.full else None
            match.append(chk["match"] if chk else None)
        ranks = {"local_ms": loc, "kernel_busy_ms": [round(r[1], 3) for r in per_rank],
                 "local_ms_min": min(loc), "local_ms_max": max(loc),
                 "spread_pct": round(100.0 * (max(loc) - min(loc)) / max(loc), 3),
                 "kernel_GHs": [round(r[3], 3) for r in per_rank],
                 "device": devices, "answer": answers, "match": match}
        # self-check: the winner re-hashes to the reported hash (host hm_hash)
        if args.full:
            assert _lib.host_hash(m, res[1]) == res[0], res
        return elapsed, res, step_ms, st, ranks

    def shard_of(name, r=rank):
        """(total nonces, rank r's inclusive shard or (None, None)).
        cfg2/cfg3: weak, rank r scans [r*2^32, (r+1)*2^32); cfg4: strong, the
        cost-weighted hm_partition shard of [0, 2^40)."""
        if name == "cfg4":
            sh = shard_range(0, (1 << 40) - 1, world, r, msg=WORKLOADS["cfg4"][0])
            return 1 << 40, sh if sh is not None else (None, None)
        return world * PER_GPU, (r * PER_GPU, (r + 1) * PER_GPU - 1)

    def bounds_of(name):
        return lambda r: shard_of(name, r)[1]

    total_nonces, (lo, hi) = shard_of(args.workload)
    elapsed, res, step_ms, st, ranks = measure(msg, lo, hi, args.steps, args.warmup,
                                               bounds_of(args.workload))
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, res, ranks["answer"])
    rl = roofline(st, msg, lo, hi) if rank == 0 and args.full else None

    # secondaries of the --full cfg2 run, so that run also clocks
    # BASELINE configs[2] (cfg3: 120-B message, two tail blocks, weak) and
    # configs[3] (cfg4: [0, 2^40) split over the N ranks, strong scaling --
    # the configuration the >= 7.5x north-star target is stated on)
    secondary = {}
    names = [] if (not args.full or args.workload != "cfg2" or args.no_secondary) else \
        [n.strip() for n in args.secondary.split(",") if n.strip()]
    for name in names:
        if name not in ("cfg3", "cfg4"):
            raise SystemExit(f"unknown secondary workload {name!r}")
        m2 = long120() if name == "cfg3" else WORKLOADS[name][0]
        tot2, (lo2, hi2) = shard_of(name)
        steps2, warm2 = (max(1, min(args.steps, 5)), 1) if name == "cfg3" else (1, 0)
        e2, r2, sm2, st2, rk2 = measure(m2, lo2, hi2, steps2, warm2, bounds_of(name))
        if rank == 0:
            secondary[name] = {
                "workload": WORKLOADS[name][1], "value": round(tot2 * steps2 / e2 / 1e9, 3),
                "unit": "GH/s", "scaling": "strong" if name == "cfg4" else "weak",
                "steps": steps2, "warmup": warm2,
                "ms_per_step": round(e2 / steps2 * 1e3, 3),
                "ms_per_step_median_rank0": round(sorted(sm2)[len(sm2) // 2], 3),
                "nonces_rank0": (hi2 - lo2 + 1) if lo2 is not None else 0,
                "result": {"hash": r2[0], "nonce": r2[1]},
                "result_vs_oracle": fixture_check(m2, 0, tot2 - 1, r2),
                "ranks": rk2,
                "all_ranks_match": all_match(rk2),
                "roofline": roofline(st2, m2, lo2, hi2) if lo2 is not None else None}

    # the hardware queues every process holds per GPU after the timed
    # regions (each rank: torch + its communicator + BENCH_STREAMS hipminer
    # streams), before any single-process child starts
    queues_after = None
    job_pcis = sorted({d["pci_bus_id"] for d in ranks["device"]})
    if rank == 0 and args.full:
        q = kfd_queues()
        queues_after = q if "error" in q else by_pci(q, job_pcis)

    # configs[3] once more through SURVEY §8(e)'s single-process model, on a
    # multi-GPU run: rank 0 starts two child processes in turn (host merge,
    # RCCL merge), each driving every GPU through one hipminer context under
    # a hard timeout, while the other ranks wait on the host; after every
    # timed region above.  HM_BENCH_SP_DEVICES (e.g. "0,0") runs it on a 1-GPU
    # box too (the RCCL child then gets the distinct ordinals, "0"); "off"
    # disables it.
    sp_env = os.environ.get("HM_BENCH_SP_DEVICES")
    sp_devices = None if sp_env == "off" else \
        [int(x) for x in sp_env.split(",")] if sp_env else \
        (list(range(world)) if world > 1 and backend == "nccl" else None)
    single = None
    if sp_devices and "cfg4" in names:
        # every rank's own context is done: closing it releases its HIP
        # streams (hardware queues), so the GPUs the children drive carry no
        # idle queues of this process's hipminer context.  The other ranks
        # wait on the host (a gloo group with a timeout), so no RCCL barrier
        # kernel spins on those GPUs either.
        ctx.close()
        wait_group = None
        if dist is not None:
            try:
                import datetime
                wait_group = dist.new_group(backend="gloo",
                                            timeout=datetime.timedelta(seconds=4 * SP_TIMEOUT_S))
            except Exception:  # no gloo: the default (device) barrier
                wait_group = None
        barrier()
        if rank == 0:
            seen = torch.cuda.device_count()
            if max(sp_devices) >= seen:
                single = {"devices": sp_devices, "skipped": f"rank 0 sees {seen} GPU(s)"}
            else:
                sp_pcis = set()
                for d in set(sp_devices):
                    pr = torch.cuda.get_device_properties(d)
                    sp_pcis.add(f"{pr.pci_domain_id:04x}:{pr.pci_bus_id:02x}:"
                                f"{pr.pci_device_id:02x}.0")
                single = run_single_process(sp_devices,
                                            list(range(world)) if backend == "nccl" else [0] * world,
                                            pcis=sp_pcis)
        if wait_group is not None:
            dist.barrier(group=wait_group)
        barrier()

    if rank == 0:
        total = total_nonces * args.steps
        value = total / elapsed / 1e9
        line = {
            "metric": "GH/s (SHA-256 nonce search) at 1/2/4/8 MI355X; % of INT32 VALU roofline",
            "value": round(value, 3),
            "unit": "GH/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3),
            "ms_per_step_median_rank0": round(sorted(step_ms)[len(step_ms) // 2], 3),
            "higher_is_better": True,
            "scaling": "strong" if args.workload == "cfg4" else "weak",
            "vs_baseline": None,
            "dtype": "u32",
            "data": "synthetic (fixed message, contiguous nonce ranges; no dataset)",
            "config": {"workload": desc, "nonces_per_gpu": total_nonces // world,
                       "parallelism": f"dp{world} (nonce shards)",
                       "hip_streams_per_gpu": BENCH_STREAMS,
                       "merge": ("RCCL all-gather" if backend == "nccl" else backend)
                                if dist is not None else "none (1 rank)"},
            "full": args.full,
            "result": {"hash": res[0], "nonce": res[1]},
            # the checks against the oracle fixtures, the roofline and the
            # queue counts are --full's (null without it)
            "result_vs_oracle": fixture_check(msg, 0, total_nonces - 1, res) if args.full
            else None,
            "ranks": ranks,
            "all_ranks_match": all_match(ranks),
            "build_id": build["build_id"],
            "build_matches_tree": build["build_matches_tree"],
            "roofline": rl,
        }
        if args.dump_outputs:
            line["outputs"] = args.dump_outputs
        if secondary:
            line["workloads"] = secondary
        line["queues_per_gpu"] = queues_after
        if single is not None:
            line["single_process"] = single
        if world == 1 and args.full and not args.no_cpu_baseline:
            cb = cpu_baseline(msg, args.workload)
            line["cpu_baseline"] = cb
        os.write(json_fd, (json.dumps(line) + "\n").encode())
        # a wrong answer fails the run (after the line is out, so the
        # mismatching rank and device are on record)
        wrong = wrong_answers(line)
        if wrong:
            print(f"bench: answers differ from the oracle fixtures: {wrong}", file=sys.stderr)
            exit_code = 1
    ctx.close()
    if dist is not None:
        dist.destroy_process_group()
    if exit_code:
        sys.exit(exit_code)


if __name__ == "__main__":
    if "--sp-child" in sys.argv:  # a single-process child (run_single_process)
        ap = argparse.ArgumentParser()
        ap.add_argument("--sp-child", choices=("host", "rccl"), required=True)
        ap.add_argument("--sp-devices", required=True)
        a = ap.parse_args()
        _sp_child_main(a.sp_child, a.sp_devices)
    else:
        main()
