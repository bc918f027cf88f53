#!/usr/bin/env python3
"""bench.py -- LLICTI encode+decode throughput on MI355X (BASELINE.json metric: MPix/s encode+decode).

    python bench.py --gpus N --steps K --warmup W

N > 1 needs no external launcher: when WORLD_SIZE is unset the parent process -- before it imports torch or touches
the GPU -- starts `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ...` as a
CHILD, relays rank 0's JSON line and exits with the child's code.  Under an external torch.distributed.run the ranks
are used as they are.

A "step" is one pass of the hot path over one batch of synthetic input on every rank: encode the batch (uint8 RGB
resident in HBM -> containers in HBM) and decode it again (containers -> uint8 RGB in HBM).  Workload at N = 1..4:
24 x 768x512 RGB per GPU (BASELINE.json configs[2], the shape the north-star target is quoted on); at N = 8:
32 per GPU = configs[4]'s 256 images over 8 GPUs.  i.i.d. uniform noise, seeds rank*B .. rank*B+B-1, weights =
seed-1337 default init (the reference does the same when its checkpoint is missing).  Images
shard across ranks with no data-path collective ("weak" scaling): the only collectives are the RCCL probe, the timing
barrier and a MAX / SUM of scalars at the end.

A plain run sets up, checks one encode + decode for losslessness, warms up, times the K steps, writes the last step's outputs
(--dump-outputs DIR) and prints one JSON line from rank 0 with the headline alone:
  value                 pixels of all ranks x K / max-over-ranks time of the K steps, inputs and outputs RESIDENT in HBM
  ms_per_step           the max-over-ranks time of the K steps / K
Everything below is measured only with --full (as every run did before that option existed):
  enc_mpix_s, dec_mpix_s  encode and decode timed apart
  value_pcie_inclusive  the same steps with H2D of the uint8 RGB, D2H of the containers (encode) and H2D of the containers,
                        D2H of the RGB (decode) inside the timed region, pinned host buffers (SURVEY.md 8(d)'s wording),
                        transfers overlapped with compute on their own HIP streams; value_pcie_serial: not overlapped
  roofline              the dominant kernel (fp32-MFMA interpolator CNN): algorithmic FLOP of the launches of one
                        encode+decode / their summed HIP-event durations (events on the launch stream, extra profiled steps)
  roofline_cdf_table    configs[3]: the full-table CDF kernel on one 3840x2160 image, SURVEY 8(d)'s bytes (2 Lp + 60 per symbol)
  coder                 SURVEY 8(d): coded symbols per second of the entropy coder's own kernels (profiled encode / decode of the run)
  bpp_delta_vs_reference, m_sweep, ac_container, ac_container_large, single_image, image_4k, natural_like, model_drawn
                        informational legs, N = 1 only, outside the timed region
  cpu_baseline          the CPU oracle in the reference's structure on the host cores, bounded sample; .torch_cpu: the same path
                        on plain PyTorch CPU ops (one image)
  n1_companion          N > 1: rank 0's solo run of the same per-GPU batch (efficiency_like_for_like)
The --no-* options below trim a --full run.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MAC_PER_POSITION = 193248            # 84,480 layer-0 + 92,928 mid + 15,840 out
PEAK_FP32_MATRIX_TFLOPS = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_16x16x4_f32, dense
PEAK_HBM_GBS = 8000.0
DEFAULT_CONTAINER = "auto"           # rANS xwide streams (256 lanes, v4 layout), their number per image a function of the image's SIZE alone: default_container(H, W)


def default_container(H, W):
    """The timed container: llicti_amd.codec.auto_container -- what LLICTI(config.container = "auto") and LLICTIAgent.eval_model use too.  It depends on
    the image size only (768x512: xrans16), not on the batch, the device or the rank count: the N = 8 run times the SAME container as N = 1."""
    from llicti_amd.codec import auto_container
    return auto_container(H, W)


def default_streams(H, W):
    from llicti_amd.codec import image_streams
    return image_streams(H, W)


NORTH_STAR_MPIX_S = 200.0            # BASELINE.json north_star: >= 200 MPix/s encode+decode on 768x512 at 1 MI355X ...
NORTH_STAR_DBPP = 0.001              # ... with bpp within 0.001 of the reference
MAC_PER_BAND = (352 * 48 + 30976 + 5280, 352 * 72 + 30976 + 5280, 352 * 120 + 30976 + 5280)   # layer 0 (K = 48 / 72 / 120) + 4 x 88 x 88 + 4 x 15 x 88
IMAGE_4K_MODES = ("xrans128", "xrans64", "xrans32", "rans128", "rans64", "rans32", "wrans14", "xrans14")   # configs[3] leg: every mode gets its Delta bpp; the headline is the fastest within 0.001 bpp
IMAGE_4K_HEADLINE = "xrans128"       # ... which tests/test_hip_parity.py::test_4k_image_oracle_parity checks against the oracle (the leg says if another mode won)
LARGE_AC_BATCH = 512                 # the batch at which the reference-format container is also measured (untimed leg): >= 1536 streams in flight
DUMP_SAMPLE = 1 << 22                # --dump-outputs: values kept of a larger output (16 MB as float32; two such arrays stay under 64 MB)
DUMP_SEED = 20240607                 # ... at these seeded positions


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=0, help="images per GPU per step (default: 24; 32 at --gpus 8 = BASELINE.json configs[4])")
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--container", default=DEFAULT_CONTAINER, help="auto (rANS xwide v4 streams, their number per image from the image size: default_container()), rans<M> / wrans<M> / xrans<M> (M streams of 64 / 128 / 256 lanes per image) or ac (torchac-compatible)")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beyond the headline: encode / decode apart, the PCIe-inclusive legs, the profiled kernel "
                         "timings (roofline, coder), the reference-format container and north-star check, the informational legs, the CPU baselines "
                         "and, at N > 1, rank 0's solo companion run")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last step computed (rank 0's batch) to DIR/<name>.npy in float32 / float64: "
                         "the decoded RGB and the container bytes (a fixed, seeded sample of each when larger than DUMP_SAMPLE values) and the segment lengths")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-torch-cpu", action="store_true", help="skip the PyTorch-CPU run of one image inside cpu_baseline (10-25 s)")
    ap.add_argument("--no-extras", action="store_true", help="skip the untimed informational legs (profiling runs)")
    ap.add_argument("--no-n1-companion", action="store_true", help="N > 1: skip rank 0's solo run of the same batch before the group forms (efficiency_like_for_like is then null)")
    ap.add_argument("--no-pcie-legs", action="store_true",
                    help="profiling runs: skip the PCIe-inclusive legs (their cross-stream waits land inside the traced durations of each call's first kernels); the line's value_pcie_* are null")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend for N > 1 (nccl = RCCL; gloo for rehearsals)")
    ap.add_argument("--no-ac-leg", action="store_true",
                    help="profiling runs: skip the (untimed) reference-format container of the batch; the line then has no bpp_delta_vs_reference / meets_north_star")
    ap.add_argument("--allow-shared-gpu", action="store_true",
                    help="let several ranks share one GPU when the node has fewer GPUs than --gpus (rehearsal only: the line is marked shared_gpu)")
    ap.add_argument("--dry-run", action="store_true",
                    help="launch / rendezvous / aggregation only, no GPU work (CPU test of the N > 1 path); prints a line with metric 'dry_run'")
    return ap.parse_args(argv)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_children(args, argv):
    """N > 1 from a bare shell: this process has not imported torch and never touches the GPU; the ranks are children."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "8")
    proc = subprocess.run(cmd, env=env)
    return proc.returncode


def positions_per_image(H, W):
    n = 0
    for lvl in range(5):
        st = 1 << lvl
        Hl, Wl = (H + st - 1) // st, (W + st - 1) // st
        n += ((Hl + 1) // 2) * ((Wl + 1) // 2)
    return n


def level_positions(H, W, lvl):
    st = 1 << lvl
    Hl, Wl = (H + st - 1) // st, (W + st - 1) // st
    return ((Hl + 1) // 2) * ((Wl + 1) // 2)


def make_batch(B, H, W, seed0):
    import numpy as np
    return np.stack([np.random.default_rng(seed0 + i).integers(0, 256, size=(3, H, W), dtype=np.uint8) for i in range(B)])


def dump_outputs(out_dir, rec, cont, seg):
    """--dump-outputs: what a caller of the timed step receives from its last run -- the decoded RGB (decode) and the containers with their
    segment lengths (encode) -- as .npy in float32 / float64, so that two builds can be compared output for output.  An output of more than
    DUMP_SAMPLE values is sampled at DUMP_SEED's sorted positions (with replacement); the container bytes are image by image the first
    seg.sum() bytes of its row (what llicti_amd.codec.container_to_bytestream_list reads), concatenated."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    rng = np.random.default_rng(DUMP_SEED)

    def sample(flat):
        if flat.size <= DUMP_SAMPLE:
            return flat
        return flat[np.sort(rng.integers(0, flat.size, size=DUMP_SAMPLE))]
    seg_h = seg.cpu().numpy()
    cont_h = cont.cpu().numpy()
    used = np.concatenate([cont_h[b, :int(n)] for b, n in enumerate(seg_h.sum(axis=1))])
    files = {"decoded_rgb": sample(rec.cpu().numpy().reshape(-1)).astype(np.float32),
             "container_bytes": sample(used).astype(np.float32),
             "segment_lengths": seg_h.astype(np.float64)}
    for name, a in files.items():
        np.save(os.path.join(out_dir, f"{name}.npy"), a)


def _latest_profile_json(name):
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", name)))
    if not files:
        return None, None
    try:
        with open(files[-1]) as fh:
            return json.load(fh), os.path.relpath(files[-1], ROOT)
    except Exception:
        return None, None


def pmc_field(kernel, field):
    d, _ = _latest_profile_json("pmc_traffic.json")
    try:
        return d[kernel][field]
    except Exception:
        return None


def cnn_rocprof():
    """Band-CNN time per step from the committed rocprofv3 kernel trace of this round's build (profiles/<round>/cnn_rocprof.json, written by
    tools/cnn_rocprof.py from the *_kernel_stats.csv of `bench.py --no-extras --no-pcie-legs`): the un-perturbed figure next to the bench's
    own event-based one.  None when not committed."""
    d, path = _latest_profile_json("cnn_rocprof.json")
    if not d:
        return None
    d = dict(d)
    d["source"] = path
    return d


def pmc_traffic(kernel="band_params_kernel"):
    """HBM bytes per launch of a kernel from rocprofv3 PMC passes (FETCH_SIZE and WRITE_SIZE in separate passes, FETCH_SIZE
    doubled per MI355X_MICROARCH.md "HBM"; tools/collect_pmc.sh + tools/pmc_traffic.py, committed as
    profiles/<round>/pmc_traffic.json -- counters cannot be read from inside this process).  None when not committed."""
    d, _ = _latest_profile_json("pmc_traffic.json")
    try:
        return d[kernel]["hbm_bytes_per_launch"]
    except Exception:
        return None


def cpu_weights():
    """The bench weights (seed-1337 default init) for the CPU oracle."""
    from llicti_amd.config import default_config
    from llicti_amd.graphs.models.LLICTI_nets import LLICTI
    from llicti_amd.weights import pack_state_dict
    from oracle import oracle as orc
    import torch
    torch.manual_seed(1337)
    return orc.Weights(pack_state_dict(LLICTI(default_config()).state_dict()))


def host_cpu():
    """(model name of the host CPU from /proc/cpuinfo, logical CPUs the process may use): SURVEY.md 8(d) asks for both beside the CPU baseline."""
    model = None
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.lower().startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    return model, (len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1))


def cpu_baseline(H, W):
    """Oracle ("port": C + OpenMP restatement in the reference's structure), on a bounded sample of the same workload."""
    import numpy as np
    from oracle import oracle as orc
    Wt = cpu_weights()
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    cores = min(cores, 64)        # the oracle's OpenMP loops stop scaling well before that
    orc.set_threads(cores)
    # bounded sample: whole images of the same workload until >= 10 s of CPU work (at most 8 images)
    n_img, t_enc, t_dec, bl0 = 0, 0.0, 0.0, None
    while n_img < 8 and t_enc + t_dec < 10.0:
        rgb = make_batch(1, H, W, n_img)[0]
        t0 = time.time()
        bl = orc.encode_image(rgb, Wt, full_tables=True)
        t1 = time.time()
        rec = orc.decode_image(bl, Wt, full_tables=True)
        t2 = time.time()
        assert np.array_equal(rec, rgb)
        t_enc += t1 - t0
        t_dec += t2 - t1
        if bl0 is None:
            bl0 = bl
        n_img += 1
    return {"value": round(n_img * H * W / 1e6 / (t_enc + t_dec), 5), "unit": "MPix/s", "cores": cores, "kind": "port",
            "sample": f"{n_img} images {W}x{H} uniform-noise RGB (seeds 0..{n_img - 1}), encode {t_enc:.2f}s + decode {t_dec:.2f}s, "
                      "C/OpenMP oracle: materialised Lp-entry tables (OpenMP over positions) + single-thread range coder",
            "enc_s": round(t_enc, 3), "dec_s": round(t_dec, 3), "cpu_model": host_cpu()[0], "host_logical_cpus": host_cpu()[1]}, bl0


def cpu_baseline_torch(H, W):
    """The north star's wording, literally: a PyTorch-CPU run of the same path (oracle/torch_cpu.py: conv2d interpolator, materialised
    [positions, 5, Lp] erfc tables, int16 integerisation, single-thread range coder -- the reference's structure on torch CPU ops),
    ONE image of the workload, encode + decode, lossless checked.  Reported inside cpu_baseline as `torch_cpu`."""
    import numpy as np
    import torch
    from llicti_amd.config import default_config
    from llicti_amd.graphs.models.LLICTI_nets import LLICTI
    from oracle import torch_cpu as tc
    torch.manual_seed(1337)
    sd = {k: v.detach().cpu() for k, v in LLICTI(default_config()).state_dict().items()}
    threads = min(len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1), 64)
    old = torch.get_num_threads()
    torch.set_num_threads(threads)
    try:
        rgb = make_batch(1, H, W, 0)[0]
        t0 = time.time()
        streams, meta = tc.encode(rgb, sd)
        t1 = time.time()
        rec = tc.decode(streams, meta, sd)
        t2 = time.time()
    finally:
        torch.set_num_threads(old)
    assert np.array_equal(rec, rgb), "PyTorch-CPU baseline: decode(encode(x)) != x"
    return {"value": round(H * W / 1e6 / (t2 - t0), 5), "unit": "MPix/s", "cores": threads, "kind": "port",
            "sample": f"1 image {W}x{H} uniform-noise RGB (seed 0), encode {t1 - t0:.2f}s + decode {t2 - t1:.2f}s, plain PyTorch CPU ops "
                      "(F.conv2d, torch.erfc tables) + single-thread C range coder in place of torchac",
            "enc_s": round(t1 - t0, 3), "dec_s": round(t2 - t1, 3), "stream_bytes": int(sum(len(x) for x in streams))}


class Legs:
    """Untimed informational legs on rank 0 at N = 1.  Every leg checks decode(encode(x)) == x on a POISONED workspace."""

    def __init__(self, torch, codec, dev):
        self.torch, self.codec, self.dev = torch, codec, dev

    def run(self, rgb, mode, reps=2, keep=False):
        torch, codec = self.torch, self.codec
        B, _, H, W = rgb.shape
        cont, seg = codec.encode(rgb, mode=mode)
        codec.check()
        dmode = mode
        if mode & 0x10000:                      # "auto": the encoder picked the counts; the decoder takes them from the headers (one per call here)
            dm = sorted(set(codec.container_modes(cont)))
            assert len(dm) == 1, dm
            dmode = dm[0]
        codec.poison_workspace()
        rec = codec.decode(cont, seg, H, W, mode=dmode)
        codec.check()
        assert torch.equal(rec, rgb), "decode(encode(x)) != x"

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / reps
        te = timed(lambda: codec.encode(rgb, mode=mode, out=cont, seg_len=seg))
        td = timed(lambda: codec.decode(cont, seg, H, W, mode=dmode, out=rec))
        mp = B * H * W / 1e6
        nbytes = int(seg.sum().item())
        r = {"batch": B, "enc_mpix_s": round(mp / te, 2), "dec_mpix_s": round(mp / td, 2), "encdec_mpix_s": round(mp / (te + td), 2),
             "enc_ms": round(te * 1e3, 3), "dec_ms": round(td * 1e3, 3), "bpp": round(8.0 * nbytes / (B * H * W), 5), "bytes": nbytes}
        if mode & 0x10000:
            from llicti_amd.codec import name_of_mode
            r["container_out"] = name_of_mode(dmode)
        if keep:
            return r, cont, seg
        return r

    def free(self):
        self.codec._ws = None
        self.torch.cuda.empty_cache()


def overlap_leg(torch, dev, sd, rgb, mode, steps=6):
    """A server that encodes one batch while it decodes another: two contexts on two HIP streams, encode(batch k) next to
    decode(containers of batch k - 1).  Same work per step as the timed step (one encode + one decode of a full batch);
    the rANS stages of the decode are latency bound and leave most of the chip to the other stream's CNN launches.
    Informational: `value` stays the un-overlapped step."""
    from llicti_amd.codec import HipCodec
    B, _, H, W = rgb.shape
    ce, cd = HipCodec(dev), HipCodec(dev)
    ce.load_state_dict(sd)
    cd.load_state_dict(sd)
    se, sdec = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    stride = ce.max_container_bytes(H, W)
    cont = [torch.empty((B, stride), dtype=torch.uint8, device=dev) for _ in range(2)]
    seg = [torch.zeros((B, 49), dtype=torch.int32, device=dev) for _ in range(2)]
    rec = torch.empty_like(rgb)
    done = [torch.cuda.Event(), torch.cuda.Event()]

    def enc(k):
        with torch.cuda.stream(se):
            ce.encode(rgb, mode=mode, out=cont[k & 1], seg_len=seg[k & 1])
            done[k & 1].record(se)

    def dec(k):
        with torch.cuda.stream(sdec):
            sdec.wait_event(done[k & 1])
            cd.decode(cont[k & 1], seg[k & 1], H, W, mode=mode, out=rec)
    torch.cuda.synchronize()
    enc(0)
    for k in range(1, 3):                   # warm-up: plans, workspaces
        enc(k)
        dec(k - 1)
    torch.cuda.synchronize()
    assert torch.equal(rec, rgb)
    t0 = time.perf_counter()
    for k in range(3, 3 + steps):
        enc(k)
        dec(k - 1)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    with torch.cuda.stream(se):
        ce.check()
    with torch.cuda.stream(sdec):
        cd.check()
    assert torch.equal(rec, rgb)
    ce.close()
    cd.close()
    return {"workload": f"{B}x{W}x{H}: encode of batch k on one HIP stream next to decode of batch k-1 on another (two contexts)",
            "encdec_mpix_s": round(B * H * W / dt / 1e6, 2), "ms_per_step": round(dt * 1e3, 3)}


class PciePipeline:
    """The step's four transfers OVERLAPPED with compute: uploads on one HIP stream, downloads on another, double buffers, events
    between them; the compute stream runs encode(k), then decode(k - 1) whose containers have meanwhile made the round trip over the
    host.  Steady-state throughput of a server fed from and draining to host memory.  run(n, trace=True) also brackets every
    operation with timing events on its own stream and returns their (start, end) in ms since the run's first event
    (tools/pcie_timeline.py)."""

    def __init__(self, torch, codec, dev, mode, rgb, cont, seg, rec, rgb_pin, cont_pin, seg_pin, rec_pin):
        self.torch, self.codec, self.dev, self.mode = torch, codec, dev, mode
        self.H, self.W = rgb.shape[2], rgb.shape[3]
        self.rgb_pin = rgb_pin
        self.s_in, self.s_out = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
        self.rgb_d = [rgb, torch.empty_like(rgb)]
        self.cont_d, self.seg_d = [cont, torch.empty_like(cont)], [seg, torch.empty_like(seg)]
        self.cont_i, self.seg_i = [torch.empty_like(cont), torch.empty_like(cont)], [torch.empty_like(seg), torch.empty_like(seg)]
        self.rec_d = [rec, torch.empty_like(rec)]
        self.cont_p = [cont_pin, torch.empty_like(cont_pin).pin_memory()]
        self.seg_p = [seg_pin, torch.empty_like(seg_pin).pin_memory()]
        self.rec_p = [rec_pin, torch.empty_like(rec_pin).pin_memory()]

    def run(self, n, trace=False):
        torch, codec, mode, H, W = self.torch, self.codec, self.mode, self.H, self.W
        s_cmp, s_in, s_out = torch.cuda.current_stream(), self.s_in, self.s_out
        E = lambda: [torch.cuda.Event(), torch.cuda.Event()]
        ev_up, ev_rgb_free, ev_enc, ev_d2h, ev_h2d, ev_dec, ev_down = E(), E(), E(), E(), E(), E(), E()
        rgb_d, cont_d, seg_d, cont_i, seg_i, rec_d = self.rgb_d, self.cont_d, self.seg_d, self.cont_i, self.seg_i, self.rec_d
        cont_p, seg_p, rec_p, rgb_pin = self.cont_p, self.seg_p, self.rec_p, self.rgb_pin
        spans = []                                   # (name, step, start event, end event)

        class Span:                                  # timing events around one operation, on the stream it is issued to
            def __init__(sp, name, k, stream):
                sp.name, sp.k, sp.stream = name, k, stream

            def __enter__(sp):
                if trace:
                    sp.e0 = torch.cuda.Event(enable_timing=True)
                    sp.e0.record(sp.stream)

            def __exit__(sp, *a):
                if trace:
                    e1 = torch.cuda.Event(enable_timing=True)
                    e1.record(sp.stream)
                    spans.append((sp.name, sp.k, sp.e0, e1))
        base = None
        if trace:
            base = torch.cuda.Event(enable_timing=True)
            base.record(s_cmp)
            s_in.wait_event(base)
            s_out.wait_event(base)

        def upload(k):
            b = k & 1
            with torch.cuda.stream(s_in):
                s_in.wait_event(ev_rgb_free[b])
                with Span("h2d_rgb", k, s_in):
                    rgb_d[b].copy_(rgb_pin, non_blocking=True)
                ev_up[b].record(s_in)

        def encode(k):
            b = k & 1
            s_cmp.wait_event(ev_up[b])
            s_cmp.wait_event(ev_d2h[b])                # cont_d[b] of step k - 2 has left for the host
            with Span("encode", k, s_cmp):
                codec.encode(rgb_d[b], mode=mode, out=cont_d[b], seg_len=seg_d[b])
            ev_enc[b].record(s_cmp)
            ev_rgb_free[b].record(s_cmp)

        def roundtrip(k):
            b = k & 1
            with torch.cuda.stream(s_out):
                s_out.wait_event(ev_enc[b])
                with Span("d2h_containers", k, s_out):
                    cont_p[b].copy_(cont_d[b], non_blocking=True)
                    seg_p[b].copy_(seg_d[b], non_blocking=True)
                ev_d2h[b].record(s_out)
            with torch.cuda.stream(s_in):
                s_in.wait_event(ev_d2h[b])
                s_in.wait_event(ev_dec[b])             # cont_i[b] of step k - 2 has been decoded
                with Span("h2d_containers", k, s_in):
                    cont_i[b].copy_(cont_p[b], non_blocking=True)
                    seg_i[b].copy_(seg_p[b], non_blocking=True)
                ev_h2d[b].record(s_in)

        def decode(k):
            b = k & 1
            s_cmp.wait_event(ev_h2d[b])
            s_cmp.wait_event(ev_down[b])               # rec_d[b] of step k - 2 has left for the host
            with Span("decode", k, s_cmp):
                codec.decode(cont_i[b], seg_i[b], H, W, mode=mode, out=rec_d[b])
            ev_dec[b].record(s_cmp)
            with torch.cuda.stream(s_out):
                s_out.wait_event(ev_dec[b])
                with Span("d2h_rgb", k, s_out):
                    rec_p[b].copy_(rec_d[b], non_blocking=True)
                ev_down[b].record(s_out)
        upload(0)
        for k in range(n):
            if k + 1 < n:
                upload(k + 1)
            encode(k)
            roundtrip(k)
            if k > 0:
                decode(k - 1)
        decode(n - 1)
        torch.cuda.synchronize()
        last = rec_p[(n - 1) & 1]
        if trace:
            return last, [{"op": nm, "step": k, "start_ms": round(base.elapsed_time(e0), 4), "end_ms": round(base.elapsed_time(e1), 4)} for nm, k, e0, e1 in spans]
        return last


def summarize_pcie_spans(spans, skip=2):
    """bench.PciePipeline.run(trace=True) spans -> where the pipelined step goes: the compute stream's period (encode(k) start to
    encode(k + 1) start), its idle gaps between consecutive compute calls, every operation's duration inside the pipeline."""
    import statistics
    ops = {}
    for sp in spans:
        ops.setdefault(sp["op"], []).append(sp)
    inside = {k: round(statistics.median(s["end_ms"] - s["start_ms"] for s in sorted(v, key=lambda s: s["step"])[skip:]), 4) for k, v in ops.items()}
    enc = sorted(ops["encode"], key=lambda s: s["step"])
    calls = sorted(ops["encode"] + ops["decode"], key=lambda s: s["start_ms"])
    period = [enc[i + 1]["start_ms"] - enc[i]["start_ms"] for i in range(skip, len(enc) - 1)]
    gaps = [calls[i + 1]["start_ms"] - calls[i]["end_ms"] for i in range(2 * skip, len(calls) - 1)]
    return {"compute_period_ms": round(statistics.median(period), 4), "compute_idle_gap_ms_per_step": round(2 * statistics.median(gaps), 4),
            "compute_idle_gap_ms_max": round(max(gaps), 4), "inside_pipeline_ms": inside}


NATURAL_FIXTURE = ("natural_like_768x512", "smooth", 512, 768, 11)      # tests/golden/ref_ideal_bits.json: the reference's own tables on this image


def natural_like_leg(torch, dev, B, H, W, mode):
    """uniform noise + sigma-floor random weights is the worst case for alphabet width and far
    from natural statistics, so the same shapes are also run on a SMOOTH set (low-pass noise + gradient, seed-fixed,
    generated on the GPU) with the "trained-like" weights of tests/golden (sigma of a few grey levels): Lp and bpp
    in a natural range.  Image 0 of the set is the full-size fixture image the reference's own Python was run on in the build
    container (tests/golden/make_fixture_ideal_bits.py), so the leg carries the north star's WHOLE bpp budget on natural-like content:
    (timed container - reference-format container), measured here on the GPU, + (build's tables - reference's tables), committed."""
    import numpy as np
    from llicti_amd.codec import MODE_AC, HipCodec
    from llicti_amd.synth import make_image
    wfile = os.path.join(ROOT, "tests", "golden", "weights_trainedlike.npz")
    if not os.path.exists(wfile):
        return None
    codec = HipCodec(dev)
    codec.load_state_dict({k: v for k, v in np.load(wfile).items()})
    g = torch.Generator(device=dev).manual_seed(2024)
    x = torch.randn((B, 3, H + 32, W + 32), device=dev, generator=g)
    k = torch.ones((3, 1, 9, 9), device=dev) / 81.0
    for _ in range(2):
        x = torch.nn.functional.conv2d(x, k, padding=4, groups=3)
    x = x[:, :, 16:16 + H, 16:16 + W]
    lum = x[:, 0:1] * 900.0
    ramp = torch.linspace(-40, 40, W, device=dev)[None, None, None, :]
    img = 128 + lum + x * 250.0 + ramp + torch.randn((B, 3, H, W), device=dev, generator=g) * 2.0
    rgb = img.round().clamp(0, 255).to(torch.uint8).contiguous()
    fixture = (H, W) == NATURAL_FIXTURE[2:4]
    if fixture:
        rgb[0] = torch.from_numpy(make_image(*NATURAL_FIXTURE[1:])).to(dev)
    legs = Legs(torch, codec, dev)
    r, cont, seg = legs.run(rgb, mode, reps=3, keep=True)
    seg_t = seg.cpu().numpy().astype(np.int64)
    del cont
    r_ac, cont_ac, seg_ac = legs.run(rgb, MODE_AC, reps=1, keep=True)
    seg_a = seg_ac.cpu().numpy().astype(np.int64)
    del cont_ac
    r["reference_format"] = {k: r_ac[k] for k in ("encdec_mpix_s", "bpp", "bytes")}
    r["bpp_delta_container_batch"] = round(8.0 * (r["bytes"] - r_ac["bytes"]) / (B * H * W), 6)
    if fixture:
        fx, fx_path = _latest_profile_json("bpp_delta_fixtures.json")
        row = next((im for im in (fx or {}).get("full_size", {}).get("images", []) if im.get("image") == NATURAL_FIXTURE[0]), None)
        d_cont = 8.0 * float(seg_t[0].sum() - seg_a[0].sum()) / (H * W)
        r["bpp_delta_container_image0"] = round(d_cont, 6)
        r["reference_format_bytes_image0"] = int(seg_a[0].sum())
        if row is not None:
            # the committed row was computed by the CPU oracle on this very image: its reference-format size must be what the GPU just wrote
            r["image0_bytes_equal_committed_oracle"] = bool(row.get("reference_format_bytes") == int(seg_a[0].sum()))
            r["bpp_delta_tables_image0_committed"] = row["delta_bpp"]
            r["bpp_delta_budget_image0"] = round(abs(d_cont) + abs(row["delta_bpp"]), 6)
            r["bpp_delta_source"] = fx_path
    mm = None
    try:
        _, _, mmt = codec.lift(rgb[:1])
        mm = [int(v) for v in mmt[0].cpu().numpy()]
    except Exception:
        pass
    codec.close()
    r["workload"] = f"{B}x{W}x{H} smooth synthetic RGB, trained-like weights (tests/golden); image 0 = fixture {NATURAL_FIXTURE[0]} (seed {NATURAL_FIXTURE[4]})"
    r["chroma_range_image0"] = mm
    return r


def model_drawn_leg(torch, dev, B, H, W, mode):
    """The timed container on content as cheap as the reference's TRAINED model (its log of natural images: 1.68 bits per symbol of the last
    stage's Cg stream, exp_debug.log.1:2677-2682) -- which neither the noise batch (12.8 bits) nor the smooth set (~7) is.  No trained checkpoint
    exists in the reference tree, so the images are DRAWN FROM A MODEL: the trained-like weights of tests/golden with one live mixture component
    of sigma 0.6 grey levels, and the reference-format decoder on this GPU fed random bytes behind the headers of a noise batch emits symbols
    with exactly the model's probabilities (tools/probe_cheap_content.py).  What cheap symbols change: a stream's serial tail is ~4,700 symbols
    instead of ~620.  Reported: the timed encoder mode, xrans10 and rans10, with bytes against the reference-format container of the same batch and
    the decode's stage / tail kernel groups."""
    import numpy as np
    from llicti_amd.codec import MODE_AC, MODE_RANS, HipCodec, last_stage_bits, name_of_mode
    wfile = os.path.join(ROOT, "tests", "golden", "weights_trainedlike.npz")
    if not os.path.exists(wfile):
        return None
    sd = dict(np.load(wfile))
    for k in list(sd):
        if k.endswith("layers1toL.2.bias"):
            b = sd[k].copy()
            b[0:15] = 0.6 / 255.0
            b[30:45] = np.tile(np.array([1.0, 1e-7, 1e-7, 1e-7, 1e-7], np.float32), 3)
            sd[k] = b
        if k.endswith("layers1toL.2.weight"):
            w = sd[k].copy()
            w[0:15] = 0.0
            w[30:45] = 0.0
            sd[k] = w
    codec = HipCodec(dev)
    codec.load_state_dict(sd)
    x0 = torch.from_numpy(make_batch(B, H, W, 0)).to(dev)
    cont, seg = codec.encode(x0, mode=MODE_AC)
    codec.check()
    ch, sh = cont.cpu().numpy().copy(), seg.cpu().numpy()
    rng = np.random.default_rng(1)
    for b in range(B):
        h0, n = int(sh[b, :4].sum()), int(sh[b].sum())
        ch[b, h0:n] = rng.integers(0, 256, n - h0, dtype=np.uint8)
    x = codec.decode(torch.from_numpy(ch).to(dev), seg, H, W, mode=MODE_AC).clone()
    torch.cuda.synchronize()
    del cont, x0
    legs = Legs(torch, codec, dev)
    r_ac, _, seg_ac = legs.run(x, MODE_AC, reps=1, keep=True)
    bits = float(np.mean([last_stage_bits(row, H, W) for row in seg_ac.cpu().numpy()]))
    out = {"workload": f"{B}x{W}x{H} images drawn from a one-component model of sigma 0.6 grey levels (trained-like weights otherwise)",
           "bits_per_last_stage_symbol": round(bits, 3), "reference_trained_model_bits_per_last_stage_symbol": 1.68,
           "reference_format": {k: r_ac[k] for k in ("encdec_mpix_s", "bpp", "bytes")}}
    # `mode`: the timed ENCODER mode ("auto": the encoder picks the count from the image -- on this content it halves the size rule's count where the
    # last stage cannot fill the payloads); beside it xrans10 -- round 5's timed container, +0.0014 bpp there in its v3 layout -- and rans10 (64 lanes)
    for m in dict.fromkeys((mode, MODE_RANS(10, wide=2), MODE_RANS(10))):
        r = legs.run(x, m, reps=3)
        r["bpp_delta_vs_ac_container"] = round(8.0 * (r["bytes"] - r_ac["bytes"]) / (B * H * W), 6)
        cont, seg = codec.encode(x, mode=m)
        dm = sorted(set(codec.container_modes(cont)))[0] if (m & 0x10000) else m
        codec.set_profiling(True)
        codec.decode(cont, seg, H, W, mode=dm)
        torch.cuda.synchronize()
        cat, _ = codec.last_timing_detail()
        codec.set_profiling(False)
        r["decode_kernel_ms"] = {k: round(v, 3) for k, v in cat.items() if v > 0}
        del cont, seg
        out[name_of_mode(m)] = r
    legs.free()
    codec.close()
    return out


def api_path_leg(torch, dev, B, H, W, n_images=240):
    """the measured throughput THROUGH the drop-in API.  `n_images` synthetic images (in host memory, uint8) go through
    LLICTIAgent.eval_model with config.eval_batch = B and config.container = "auto": per batch H2D of the uint8 RGB, encode, D2H of the
    containers, container -> the reference's bytestream_list (6 lists x 9 `bytes` per image), rate bookkeeping, bytestream_list -> container,
    H2D, decode, the lossless check and the per-image log line -- everything eval_model does (agents/llicti_agent.py:122-164) inside one
    wall clock, the host half of batch k overlapped with the GPU half of batch k + 1.  Beside it the same images through an agent whose config
    has NEITHER key (what a caller gets who changes nothing but the import: the agent's defaults are that very path) and the opt-in
    reference-format one-image loop on a few images."""
    import logging
    import numpy as np
    from llicti_amd.agents.llicti_agent import LLICTIAgent
    from llicti_amd.config import default_config
    logging.getLogger("Agent").setLevel(logging.WARNING)           # 240 log lines are formatted, not printed
    imgs = [np.random.default_rng(1000 + i).integers(0, 256, size=(3, H, W), dtype=np.uint8) for i in range(n_images)]
    out = {"workload": f"{n_images} x {W}x{H} uniform-noise RGB through LLICTIAgent.eval_model, eval_batch = {B}, container auto, wall clock incl. transfers, "
                       "container <-> bytestream_list, rates, lossless check, log lines"}
    agent = LLICTIAgent(default_config(test_data=imgs[:2 * B], eval_batch=B, container="auto"))
    agent.run()                                                   # warm-up: plans, workspaces, pinned staging buffers
    agent.config["test_data"] = imgs
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = agent.run()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert len(res) == n_images and all(r["max_abs_err"] == 0.0 for r in res)
    bpsp_auto = [r["bpsp"] for r in res]
    out["batched"] = {"mpix_s": round(n_images * H * W / dt / 1e6, 2), "wall_s": round(dt, 4), "ms_per_image": round(dt / n_images * 1e3, 3),
                      "bpsp": round(float(np.mean([r["bpsp"] for r in res])), 5), "container": agent.model.container,
                      "gpu_enc_ms_per_image": round(float(np.mean([r["enc_s"] for r in res])) * 1e3, 3),
                      "gpu_dec_ms_per_image": round(float(np.mean([r["dec_s"] for r in res])) * 1e3, 3)}
    del agent
    # (a) what a caller gets who changes nothing but the import: the reference's own config has neither `container` nor `eval_batch` -- the agent then
    #     runs container "auto" with eval_batch 24 (the throughput path is the default, the reference format the opt-in) --,
    # (b) the opt-in: "container": "ac", "eval_batch": 1 = the reference's byte format in its one-image loop
    a0 = LLICTIAgent(default_config(test_data=imgs[:2 * B]))
    a0.run()
    a0.config["test_data"] = imgs
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r0 = a0.run()
    torch.cuda.synchronize()
    dt0 = time.perf_counter() - t0
    assert len(r0) == n_images and all(r["max_abs_err"] == 0.0 for r in r0)
    out["unchanged_reference_config"] = {"mpix_s": round(n_images * H * W / dt0 / 1e6, 2), "ms_per_image": round(dt0 / n_images * 1e3, 3),
                                         "what": "no container / eval_batch key in the config (configs/llicti_A.json has neither): the agent's defaults -- container auto, eval_batch 24",
                                         "bytes_equal_explicit_auto": bool([r["bpsp"] for r in r0] == bpsp_auto)}     # per image, in order
    del a0
    a1 = LLICTIAgent(default_config(test_data=imgs[:1], container="ac", eval_batch=1))
    a1.run()
    a1.config["test_data"] = imgs[:3]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r1 = a1.run()
    torch.cuda.synchronize()
    dt1 = time.perf_counter() - t0
    out["reference_format_one_image_loop"] = {"mpix_s": round(3 * H * W / dt1 / 1e6, 3), "ms_per_image": round(dt1 / 3 * 1e3, 2), "container": a1.model.container,
                                              "enc_s": round(float(np.mean([r["enc_s"] for r in r1])), 4), "dec_s": round(float(np.mean([r["dec_s"] for r in r1])), 4)}
    logging.getLogger("Agent").setLevel(logging.NOTSET)
    return out


def api_path_mixed_leg(torch, dev, B, n_images=500):
    """the drop-in API on the reference's OWN eval workload -- 500 images at the sizes its test set has, in the order its loader
    yields them (tests/golden/eval_shapes.json: parsed out of the reference's eval log, 119 distinct sizes, interleaved; the images themselves
    are not in the reference tree, so the content is the bench's uniform noise) -- through LLICTIAgent.eval_model with eval_batch = B and
    container "auto": every batch is B CONSECUTIVE images whatever their sizes (llicti_encode_images_v / llicti_decode_images_v), wall clock
    with everything eval_model does inside.  Beside it: the same images grouped the round-4 way (a batch closes where the size changes)."""
    import logging
    import numpy as np
    from llicti_amd.agents.llicti_agent import LLICTIAgent
    from llicti_amd.config import default_config
    shapes = json.load(open(os.path.join(ROOT, "tests", "golden", "eval_shapes.json")))["shapes"][:n_images]
    logging.getLogger("Agent").setLevel(logging.WARNING)
    imgs = [np.random.default_rng(5000 + i).integers(0, 256, size=(3, h, w), dtype=np.uint8) for i, (h, w) in enumerate(shapes)]
    pix = float(sum(h * w for h, w in shapes))
    out = {"workload": f"{len(shapes)} uniform-noise RGB images at the sizes and in the order of the reference's own test set ({len(set(map(tuple, shapes)))} distinct sizes, "
                       f"{pix / 1e6:.1f} MPix) through LLICTIAgent.eval_model, eval_batch = {B}, container auto, wall clock incl. transfers, container <-> bytestream_list, "
                       "rates, lossless check, log lines"}
    agent = LLICTIAgent(default_config(test_data=imgs[:3 * B], eval_batch=B, container="auto"))
    agent.run()                                                   # warm-up: workspaces, pinned staging buffers, table blocks
    agent.config["test_data"] = imgs
    dts = []
    for _ in range(3):                                            # a wall clock over host threads, copies and kernels: median of three, spread in the line
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = agent.run()
        torch.cuda.synchronize()
        dts.append(time.perf_counter() - t0)
    dt = sorted(dts)[1]
    out["repeats_mpix_s"] = [round(pix / t / 1e6, 1) for t in dts]
    assert len(res) == len(shapes) and all(r["max_abs_err"] == 0.0 for r in res)
    assert [(r["H"], r["W"]) for r in res] == [tuple(s) for s in shapes]              # in order
    out["stream_counts"] = ("per image: the encoder mode its own size gives (llicti_amd.codec.auto_modes -> llicti_encode_images_vm), the count picked on the device "
                            "from what the image's last stage costs -- the bytes of an image do not depend on its neighbours in the batch")
    out["mixed_batches"] = {"mpix_s": round(pix / dt / 1e6, 2), "wall_s": round(dt, 4), "ms_per_image": round(dt / len(shapes) * 1e3, 3),
                            "bpsp": round(float(np.mean([r["bpsp"] for r in res])), 5),
                            "gpu_enc_ms_per_image": round(float(np.mean([r["enc_s"] for r in res])) * 1e3, 3),
                            "gpu_dec_ms_per_image": round(float(np.mean([r["dec_s"] for r in res])) * 1e3, 3)}
    # round 4's grouping on the same images: consecutive equal sizes only (what the one-size-per-call C-ABI allowed)
    runs, cur = [], []
    for im in imgs:
        if cur and (im.shape != cur[0].shape or len(cur) == B):
            runs.append(cur)
            cur = []
        cur.append(im)
    runs.append(cur)
    out["equal_size_runs"] = {"batches": len(runs), "mean_batch": round(len(imgs) / len(runs), 2)}
    n_sub = min(len(runs), 60)
    sub = [im for r in runs[:n_sub] for im in r]
    sub_pix = float(sum(im.shape[1] * im.shape[2] for im in sub))
    model = agent.model
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for r in runs[:n_sub]:
        enc = model.encode_batch_async(r)
        rec, _, _ = model.decode_batch_async(enc.lists(check=False), dev, flat=True)
    model.codec().check()
    torch.cuda.synchronize()
    dt2 = time.perf_counter() - t0
    out["equal_size_runs"].update({"mpix_s": round(sub_pix / dt2 / 1e6, 2), "images": len(sub),
                                   "what": "the same images, a call per run of consecutive equal sizes, unpipelined encode -> lists -> decode (no rates / log lines)"})
    del agent
    logging.getLogger("Agent").setLevel(logging.NOTSET)
    return out


def table_kernel_roofline(codec, torch, H=2160, W=3840):
    """BASELINE.json configs[3]: one 3840x2160 image, the full-table CDF kernel (the reference's get_cdfs +
    _convert_to_int_and_normalize, LLICTI_nets.py:938-983) at level 0 -- HBM-write bound by construction.
    Algorithmic bytes per coded symbol: 2 * Lp written + 60 B of mixture parameters read (the row
    pitch in HBM is 264 / 512 entries and the kernel reads 256-byte CNN rows; the padding is not counted);
    duration from events on the launch stream."""
    rgb = torch.from_numpy(make_batch(1, H, W, 0)).cuda()
    planes, fplanes, mm = codec.lift(rgb)
    mm_h = [int(v) for v in mm[0].cpu().numpy()]
    params = codec.band_params(fplanes, 0, 0)
    out = {}
    tot_b, tot_ms = 0.0, 0.0
    for clr, stride in ((0, 264), (1, 512), (2, 512)):
        Lp = 257 if clr == 0 else (mm_h[2 + clr - 1] - mm_h[clr - 1] + 2)
        codec.cdf_tables(planes, params, mm, 0, 0, clr, row_stride=stride)       # warm-up
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n = 3
        tabs = None
        e0.record()
        for _ in range(n):
            tabs = None
            tabs = codec.cdf_tables(planes, params, mm, 0, 0, clr, row_stride=stride)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / n
        rows = tabs.shape[1]
        nbytes = rows * (2.0 * Lp + 60.0)
        out[("Y", "Co", "Cg")[clr]] = {"ms": round(ms, 3), "Lp": Lp, "GB_s": round(nbytes / ms / 1e6, 1)}
        tot_b += nbytes
        tot_ms += ms
        del tabs
    ach = tot_b / tot_ms / 1e6
    valu = pmc_field("cdf_table_kernel", "valu_issue_frac")
    hbm = {"achieved": round(ach, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(ach / PEAK_HBM_GBS, 4),
           "what": "SURVEY 8(d)(ii)'s algorithmic bytes (2 Lp written + 60 B read per coded symbol) over the launches' event time, against HBM peak: the bound "
                   "the survey expected, NOT the binding one"}
    # The binding roof ("VALU throughput must be shown not to be the tighter bound" -- it is): vector instructions issued per launch against
    # one wave64 instruction per SIMD every 2 cycles over the launch's cycles, from the committed PMC passes of tools/bench_table.py.  VERDICT r5 #5: the
    # record says so in `bound` / `frac`, with the HBM figure beside it.
    return {"bound": "valu" if valu is not None else "hbm", "kernel": "cdf_table_kernel",
            "achieved": (round(valu * 100.0, 2) if valu is not None else hbm["achieved"]), "peak": (100.0 if valu is not None else PEAK_HBM_GBS),
            "unit": ("% of the VALU issue slots (1,024 SIMDs x one wave64 instruction per 2 cycles)" if valu is not None else "GB/s"),
            "frac": (round(valu, 4) if valu is not None else hbm["frac"]),
            "frac_is": "SQ_INSTS_VALU per launch / (GRBM_GUI_ACTIVE / 8 XCDs x 1,024 SIMDs / 2), committed PMC passes (pmc_source); the launch time of THIS run is in hbm / per_channel",
            "hbm": hbm, "traffic": pmc_traffic("cdf_table_kernel"),
            "valu_issue_frac": (round(valu, 4) if valu is not None else None),
            "valu_insts_per_launch": pmc_field("cdf_table_kernel", "valu_insts_per_launch"),
            "pmc_source": _latest_profile_json("pmc_traffic.json")[1],
            "workload": f"{W}x{H} image, level 0 band x11: {rows} rows, Lp = 257 (Y) / per-image (Co, Cg) uint16 entries; BASELINE.json configs[3]",
            "per_channel": out, "bytes_per_launch_avg": tot_b / 3.0,
            "bytes_model": "SURVEY 8(d)(ii): 2*Lp + 60 B per coded symbol"}


def solo_companion(torch, dev, B, H, W, args):
    """Rank 0 alone on its GPU: K timed steps (encode + decode of the per-GPU batch, resident in HBM) in the container the N > 1 run times --
    the denominator of efficiency_like_for_like.  Same seeds, same weights, same code path as the timed region of main()."""
    from llicti_amd.codec import HipCodec, mode_of_name, name_of_mode
    from llicti_amd.config import default_config
    from llicti_amd.graphs.models.LLICTI_nets import LLICTI
    name = default_container(H, W) if args.container == "auto" else args.container
    mode = mode_of_name(name)
    torch.manual_seed(1337)
    codec = HipCodec(dev)
    codec.load_state_dict(LLICTI(default_config()).state_dict())
    rgb = torch.from_numpy(make_batch(B, H, W, seed0=0)).to(dev)
    cont, seg = codec.encode(rgb, mode=mode)
    codec.check()
    dmode = sorted(set(codec.container_modes(cont)))[0] if (mode & 0x10000) else mode
    rec = torch.empty_like(rgb)

    def step():
        codec.encode(rgb, mode=mode, out=cont, seg_len=seg)
        codec.decode(cont, seg, H, W, mode=dmode, out=rec)
    for _ in range(max(1, args.warmup)):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    codec.check()
    assert torch.equal(rec, rgb)
    out = {"value": round(B * H * W * args.steps / dt / 1e6, 3), "unit": "MPix/s", "batch": B, "container": name, "container_written": name_of_mode(dmode),
           "steps": args.steps, "ms_per_step": round(dt / args.steps * 1e3, 3),
           "what": "rank 0 alone on its GPU before the process group formed: the same per-GPU batch, container and step as the N > 1 run"}
    codec.close()
    del rgb, cont, seg, rec
    torch.cuda.empty_cache()
    return out


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    args = parse_args(argv)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return launch_children(args, argv)

    import numpy as np
    import torch
    import torch.distributed as dist
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} but the launcher started {world} ranks (WORLD_SIZE)")
    B = args.batch or (32 if world == 8 else 24)
    H, W = args.height, args.width

    if args.dry_run:
        # the N > 1 plumbing without a GPU: rendezvous, barrier, MAX / SUM aggregation, the per-rank gather, one line from rank 0
        from llicti_amd import shard
        if world > 1:
            dist.init_process_group("gloo" if args.backend != "nccl" or not torch.cuda.is_available() else "nccl")
        shard.barrier()
        agg = shard.aggregate(1.0 + rank, 1000 * (rank + 1), B * H * W)
        # (dry run: a made-up NUMA placement -- ranks 0 .. 3 on node 0, 4 .. 7 on node 1, 16 CPUs each -- goes through the same gather as the real one)
        per = shard.gather_per_rank([1.0 + rank, 2.0 + rank, float(rank), float(rank), float(rank // 4), 16.0])     # elapsed, pcie elapsed, device identity, local device, NUMA node, CPUs bound
        rows, straggler = shard.per_rank_report([p[0] for p in per], [p[1] for p in per], B * H * W, 1, [int(p[2]) for p in per], [int(p[3]) for p in per],
                                                numa=[(p[4], p[5]) for p in per])
        # the like-for-like N = 1 companion (below, the real path): rank 0 alone, the SAME per-GPU batch and container, before the group forms; here: rank 0's made-up second
        solo_value = B * H * W / 1.0 / 1e6
        if rank == 0:
            tag = "; BASELINE.json configs[4] (256 images sharded 32 per GPU)" if (world == 8 and B == 32 and (H, W) == (512, 768)) else ""
            print(json.dumps({"metric": "dry_run", "value": None, "n_gpus": world, "ranks_seen": dist.get_world_size() if world > 1 else 1,
                              "batch_per_gpu": B, "pixels": agg["pixels"], "bytes": agg["bytes"], "elapsed_max_s": agg["elapsed_s"],
                              "container": default_container(H, W) if args.container == "auto" else args.container,
                              "config": {"workload": f"{B}x{W}x{H} per GPU" + tag},
                              "per_rank": rows, "straggler_ratio": straggler,
                              "n1_companion": {"value": round(solo_value, 3), "batch": B, "what": "dry run: made up"},
                              "efficiency_like_for_like": round(agg["pixels"] / agg["elapsed_s"] / 1e6 / (world * solo_value), 4),
                              "distinct_devices": shard.distinct_devices([int(p[2]) for p in per])}), flush=True)
        if world > 1:
            dist.destroy_process_group()
        return 0

    n_dev = max(1, torch.cuda.device_count())
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
    shared_gpu = local_world > n_dev
    if shared_gpu and not args.allow_shared_gpu:
        raise SystemExit(f"{local_world} ranks on this node but only {n_dev} GPU(s) visible: a line with n_gpus = {world} would be read as "
                         "multi-GPU throughput; pass --allow-shared-gpu for a rehearsal of the launch path (the line then says shared_gpu: true)")
    local_dev = local_rank % n_dev                               # identity on a full node
    torch.cuda.set_device(local_dev)
    dev = torch.device("cuda", local_dev)
    # One process per GPU: this rank's host threads run on the CPUs of the NUMA node its GPU hangs off, and its pinned staging buffers -- allocated
    # below, first touched here -- lie there too (the PCIe-inclusive legs copy 172 MB per step; llicti_amd.shard.bind_to_gpu_numa).  Only where several
    # ranks share the host: a lone process keeps the affinity it was given.
    from llicti_amd import shard as _shard
    numa = _shard.bind_to_gpu_numa(dev) if world > 1 else {"numa_node": None, "cpus_bound": 0, "cpus": None}
    # N > 1: the like-for-like N = 1 companion.  Rank 0 runs the SAME per-GPU batch in the SAME container alone on its GPU
    # BEFORE the process group forms -- the other ranks sit in the rendezvous and have not touched their GPUs -- so that the line can say
    # efficiency_like_for_like = value / (N x this) without mixing batch size or container with rank count.
    n1_companion = None
    if world > 1 and rank == 0 and args.full and not args.no_n1_companion:
        n1_companion = solo_companion(torch, dev, B, H, W, args)
    rccl_ranks = 1
    if world > 1:
        # RCCL over xGMI; used for the probe, the barrier and two scalar all-reduces only (no data-path collective).
        # The backend is ONE decision for the whole job: a rank whose RCCL set-up fails exits non-zero (no per-rank fallback
        # to another backend, which would leave the ranks in different groups).
        dist.init_process_group(args.backend, **({"device_id": dev} if args.backend == "nccl" else {}))
        probe = torch.ones(1, device=dev if args.backend == "nccl" else "cpu")
        dist.all_reduce(probe)                      # forces communicator set-up now, outside any timed region
        if args.backend == "nccl":
            torch.cuda.synchronize()
        rccl_ranks = int(round(float(probe.item())))
        assert rccl_ranks == world == dist.get_world_size(), (rccl_ranks, world)

    from llicti_amd.codec import MODE_AC, MODE_RANS, HipCodec, container_to_bytestream_list
    from llicti_amd.config import default_config
    from llicti_amd.graphs.models.LLICTI_nets import LLICTI
    from llicti_amd import shard

    from llicti_amd.codec import mode_of_name as mode_of, name_of_mode
    if args.container == "auto":
        args.container = default_container(H, W)
    mode = mode_of(args.container)
    torch.manual_seed(1337)
    sd = LLICTI(default_config()).state_dict()                # seed-1337 default init, identical on every rank
    codec = HipCodec(dev)
    codec.load_state_dict(sd)

    rgb_h = make_batch(B, H, W, seed0=rank * B)
    rgb = torch.from_numpy(rgb_h).to(dev)
    stride = codec.max_container_bytes(H, W)
    cont = torch.empty((B, stride), dtype=torch.uint8, device=dev)
    seg = torch.zeros((B, 49), dtype=torch.int32, device=dev)
    rec = torch.empty_like(rgb)
    barrier = shard.barrier

    def enc():
        return codec.encode(rgb, mode=mode, out=cont, seg_len=seg)

    # Container "auto" is an ENCODER mode: the stream count of an image is picked by the encoder, on the device, from the image itself (its size
    # and what its last stage costs; llicti_amd.codec.MODE_RANS_AUTO) and written into the container's header.  A decoder reads the header -- here
    # once, outside the timed region (a real decoder gets its containers from the host and has the header before it has anything else).
    dmode = [mode]

    def dec():
        return codec.decode(cont, seg, H, W, mode=dmode[0], out=rec)

    def step():
        enc()
        dec()

    # correctness outside the timed region: lossless with the workspace poisoned between encode and decode
    enc()
    codec.check()
    if mode & 0x10000:
        got_modes = sorted(set(codec.container_modes(cont)))
        if len(got_modes) != 1:
            raise SystemExit(f"the encoder picked different stream counts for the images of the timed batch ({[name_of_mode(m) for m in got_modes]}): "
                             "the timed decode takes one mode per call -- name a container (--container xrans<M>)")
        dmode[0] = got_modes[0]
    container_out = name_of_mode(dmode[0])
    codec.poison_workspace()
    rec.zero_()
    dec()
    codec.check()
    assert torch.equal(rec, rgb), "decode(encode(x)) != x"
    seg_h = seg.cpu().numpy()
    total_bytes = int(seg_h.sum())
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n
    t_enc = t_dec = None
    if args.full:
        t_enc = timed(enc, max(1, min(3, args.steps)))
        t_dec = timed(dec, max(1, min(3, args.steps)))

    # ---- the timed region: K steps, inputs / outputs resident in HBM
    barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    barrier()
    elapsed = time.perf_counter() - t0
    codec.check()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, rec, cont, seg)

    elapsed_pcie = elapsed_pcie_serial = None
    pcie_spread, pcie_trace = None, None
    if args.full and not args.no_pcie_legs:
        # ---- the same steps with the PCIe transfers inside (pinned host buffers): never `value`, reported beside it
        rgb_pin = torch.from_numpy(rgb_h).pin_memory()
        cont_pin = torch.empty((B, stride), dtype=torch.uint8).pin_memory()
        seg_pin = torch.empty((B, 49), dtype=torch.int32).pin_memory()
        rec_pin = torch.empty((B, 3, H, W), dtype=torch.uint8).pin_memory()

        def step_pcie():
            rgb.copy_(rgb_pin, non_blocking=True)
            enc()
            cont_pin.copy_(cont, non_blocking=True)
            seg_pin.copy_(seg, non_blocking=True)
            torch.cuda.synchronize()                      # the host owns the containers here
            cont.copy_(cont_pin, non_blocking=True)
            seg.copy_(seg_pin, non_blocking=True)
            dec()
            rec_pin.copy_(rec, non_blocking=True)
            torch.cuda.synchronize()
        step_pcie()
        n_pcie = max(1, min(args.steps, 5))
        barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n_pcie):
            step_pcie()
        barrier()
        elapsed_pcie_serial = (time.perf_counter() - t0) / n_pcie
        assert np.array_equal(rec_pin.numpy(), rgb_h)

        # The same four transfers per step, OVERLAPPED with compute (PciePipeline above)
        pipe = PciePipeline(torch, codec, dev, dmode[0], rgb, cont, seg, rec, rgb_pin, cont_pin, seg_pin, rec_pin)      # (the container the timed encode writes on this batch, by name)
        pcie_pipeline = pipe.run
        pcie_pipeline(2)                                   # warm-up: second buffers, streams
        # steady state: the difference of a long and a short pipelined run (both pay the same fill and drain)
        n_short, n_long = 3, 3 + max(4, min(2 * args.steps, 16))
        est = []
        for _ in range(5):                                 # the estimator is a difference of two wall-clock runs: repeat it, keep the median, report the spread
            t_pipe = []
            for n in (n_short, n_long):
                barrier()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                last = pcie_pipeline(n)
                barrier()
                t_pipe.append(time.perf_counter() - t0)
            est.append(max(1e-9, (t_pipe[1] - t_pipe[0]) / (n_long - n_short)))
        est.sort()
        elapsed_pcie = est[len(est) // 2]
        pcie_spread = [round(B * H * W / e / 1e6, 1) for e in (est[-1], est[0])]      # slowest, fastest repeat (this rank), MPix/s
        codec.check()
        assert np.array_equal(last.numpy(), rgb_h)
        # one traced pipelined run (timing events around every transfer and compute call on its own stream): does the compute stream run
        # back to back (period = resident step, no idle gaps) or do the transfers hold it up?  Says so in every line, whatever the box.
        pcie_trace = None
        try:
            _, spans = pipe.run(3 + 6, trace=True)
            pcie_trace = summarize_pcie_spans(spans)
            pcie_trace["resident_step_ms"] = round((t_enc + t_dec) * 1e3, 4)
            pcie_trace["transfers_overlap_compute"] = bool(pcie_trace["compute_period_ms"] <= 1.03 * (t_enc + t_dec) * 1e3)
        except Exception as e:                       # diagnostics only
            pcie_trace = {"skipped": repr(e)[:200]}
        del rgb_pin, cont_pin, seg_pin, rec_pin, last, pipe, pcie_pipeline

    # ---- dominant-kernel timing with HIP events on the launch stream, in extra (untimed) profiled steps
    cnn_ms, cnn_launches, call_ms = 0.0, 0, 0.0
    kernel_ms = {}                                   # per kernel group, encode and decode pass (HIP events around the launches)
    cnn_level_ms = [0.0] * 5                         # band-CNN time per level (both passes)
    if args.full:
        codec.set_profiling(True)
        for name, fn in (("encode", enc), ("decode", dec)):
            fn()
            torch.cuda.synchronize()
            ms, n = codec.last_timing()
            cat, per = codec.last_timing_detail()
            cnn_ms += ms[1]
            cnn_launches += n
            call_ms += ms[0]
            kernel_ms[name] = {k: round(v, 3) for k, v in cat.items() if v > 0}
            kernel_ms[name]["call"] = round(ms[0], 3)
            for l, t in enumerate(codec.last_cnn_level_ms()):
                cnn_level_ms[l] += t
        codec.set_profiling(False)
    assert abs(sum(MAC_PER_BAND) - MAC_PER_POSITION) == 0

    # ---- untimed: the reference-format (torchac-compatible) container on rank 0's batch -- Delta bpp of the timed container is
    #      measured against it in EVERY --full line (meets_north_star); its first image is compared with the CPU oracle below
    legs_out = {}
    cont_ac0 = seg_ac0 = None
    ac_bytes = None
    if rank == 0 and args.full and not args.no_ac_leg:
        r_ac, cont2, seg2 = Legs(torch, codec, dev).run(rgb, MODE_AC, reps=1, keep=True)
        ac_bytes = r_ac["bytes"]
        seg_ac0 = seg2[0].cpu().numpy()
        cont_ac0 = cont2[0].cpu().numpy()
        r_ac["workload"] = f"{B}x{W}x{H}, reference-format container (45 torchac-algorithm streams per image)"
        legs_out["ac_container"] = r_ac
        del cont2, seg2
        codec._ws = None
    # ---- untimed informational legs (rank 0, N = 1 only, like cpu_baseline)
    extras = args.full and (world == 1) and not args.no_extras and not args.no_ac_leg
    if extras:
        legs = Legs(torch, codec, dev)
        # (2) rANS streams per image: speed against container overhead
        sweep = []
        for M in (1, 2, 4, 8, 10, 12, 16, 32):
            r = legs.run(rgb, MODE_RANS(M), reps=2)
            sweep.append({"M": M, "lanes": 64, "encdec_mpix_s": r["encdec_mpix_s"], "enc_mpix_s": r["enc_mpix_s"], "dec_mpix_s": r["dec_mpix_s"],
                          "bpp_delta_vs_ac_container": round(8.0 * (r["bytes"] - ac_bytes) / (B * H * W), 5)})
        for wide, Ms in ((1, (4, 6, 8, 10)), (2, (8, 10, 12, 15, 16, 18, 20, 21, 24))):      # wide streams: 128 lanes, two lanes per symbol; xwide (v4): 256 lanes, one lane per symbol
            for M in Ms:
                r = legs.run(rgb, MODE_RANS(M, wide=wide), reps=2)
                sweep.append({"M": M, "lanes": 64 << wide, "encdec_mpix_s": r["encdec_mpix_s"], "enc_mpix_s": r["enc_mpix_s"], "dec_mpix_s": r["dec_mpix_s"],
                              "bpp_delta_vs_ac_container": round(8.0 * (r["bytes"] - ac_bytes) / (B * H * W), 5)})
        legs_out["m_sweep"] = {"workload": f"{B}x{W}x{H}, rANS container with M streams per image", "modes": sweep}
        legs.free()
        # (2b) the N = 8 run's per-GPU workload (configs[4]: 32 images per GPU, its own container) on ONE GPU: what an 8-GPU value has to be divided
        #      by for a like-for-like scaling efficiency (the driver's N = 1 point is the batch of 24)
        try:
            b32 = torch.from_numpy(make_batch(32, H, W, seed0=0)).to(dev)
            r32 = legs.run(b32, mode_of(default_container(H, W)), reps=3)
            r32["container"] = default_container(H, W)
            r32["workload"] = f"32x{W}x{H} on ONE GPU: the per-GPU batch of bench.py --gpus 8 (BASELINE.json configs[4]); N = 8 efficiency like for like = value(N = 8) / (8 x this)"
            legs_out["batch32_single_gpu"] = r32
            del b32
        except Exception as e:
            legs_out["batch32_single_gpu"] = {"skipped": repr(e)[:200]}
        legs.free()
        # (3) configs[1]: ONE 768x512 image
        one = rgb[:1].contiguous()
        legs_out["single_image"] = {"workload": f"1x{W}x{H} (BASELINE.json configs[1])",
                                    "rans128": legs.run(one, MODE_RANS(128), reps=5), "rans64": legs.run(one, MODE_RANS(64), reps=5), "rans32": legs.run(one, MODE_RANS(32), reps=5),
                                    "rans16": legs.run(one, MODE_RANS(16), reps=5), "xrans64": legs.run(one, MODE_RANS(64, wide=2), reps=5),
                                    "xrans32": legs.run(one, MODE_RANS(32, wide=2), reps=5), "xrans24": legs.run(one, MODE_RANS(24, wide=2), reps=5),
                                    "xrans20": legs.run(one, MODE_RANS(20, wide=2), reps=5), "xrans15": legs.run(one, MODE_RANS(15, wide=2), reps=5),
                                    "xrans10": legs.run(one, MODE_RANS(10, wide=2), reps=5),
                                    default_container(H, W): legs.run(one, mode_of(default_container(H, W)), reps=5),      # what container "auto" gives this image
                                    "ac": legs.run(one, MODE_AC, reps=1)}
        for nm, r in legs_out["single_image"].items():
            if isinstance(r, dict) and nm != "ac":
                r["bpp_delta_vs_ac_container"] = round(r["bpp"] - legs_out["single_image"]["ac"]["bpp"], 5)
        # configs[1]'s honest headline: the fastest mode INSIDE the north star's 0.001 bpp (the 128-stream latency mode is 26x over it)
        si = legs_out["single_image"]
        ok = [nm for nm, r in si.items() if isinstance(r, dict) and nm != "ac" and abs(r.get("bpp_delta_vs_ac_container", 1.0)) <= NORTH_STAR_DBPP]
        best_si = max(ok, key=lambda nm: si[nm]["encdec_mpix_s"]) if ok else None
        fastest = max((nm for nm, r in si.items() if isinstance(r, dict) and nm != "ac"), key=lambda nm: si[nm]["encdec_mpix_s"])
        si["in_budget"] = ({"container": best_si, "encdec_mpix_s": si[best_si]["encdec_mpix_s"], "bpp_delta_vs_ac_container": si[best_si]["bpp_delta_vs_ac_container"],
                            "meets_200_mpix_s": bool(si[best_si]["encdec_mpix_s"] >= NORTH_STAR_MPIX_S)} if best_si else None)
        si["fastest_any_size"] = {"container": fastest, "encdec_mpix_s": si[fastest]["encdec_mpix_s"], "bpp_delta_vs_ac_container": si[fastest]["bpp_delta_vs_ac_container"]}
        legs.free()
        # (4) the reference-format container where it has enough streams in flight
        try:
            big = torch.from_numpy(make_batch(LARGE_AC_BATCH, H, W, seed0=0)).to(dev)
            r, cbig, sbig = legs.run(big, MODE_AC, reps=1, keep=True)
            n0 = int(seg_ac0.sum())
            assert np.array_equal(cbig[0, :n0].cpu().numpy(), cont_ac0[:n0]), "image 0 coded in the large batch differs from image 0 coded in a batch of 24"
            r["workload"] = f"{LARGE_AC_BATCH}x{W}x{H} on ONE GPU, reference-format container"
            legs_out["ac_container_large"] = r
            r = legs.run(big, MODE_RANS(1), reps=1)
            r["bpp_delta_vs_ac_container"] = round(r["bpp"] - legs_out["ac_container_large"]["bpp"], 5)
            r["workload"] = f"{LARGE_AC_BATCH}x{W}x{H} on ONE GPU, rANS container with ONE stream per image"
            legs_out["rans1_large"] = r
            del big, cbig, sbig
        except torch.cuda.OutOfMemoryError as e:      # a smaller card: skip, say so
            legs_out["ac_container_large"] = {"skipped": repr(e)[:200]}
        legs.free()
        # (5) configs[3] end to end: one 3840x2160 image
        big = torch.from_numpy(make_batch(1, 2160, 3840, seed0=0)).to(dev)
        r4k_ac = legs.run(big, MODE_AC, reps=1)
        modes4k = {}
        for nm in IMAGE_4K_MODES:
            r = legs.run(big, mode_of(nm), reps=2)
            r["bpp_delta_vs_ac_container"] = round(8.0 * (r["bytes"] - r4k_ac["bytes"]) / (2160 * 3840), 6)
            modes4k[nm] = r
        in_budget = [nm for nm in IMAGE_4K_MODES if abs(modes4k[nm]["bpp_delta_vs_ac_container"]) <= NORTH_STAR_DBPP]
        best = max(in_budget, key=lambda nm: modes4k[nm]["encdec_mpix_s"]) if in_budget else None
        legs_out["image_4k"] = {"workload": "1x3840x2160 uniform-noise RGB (BASELINE.json configs[3]) end to end",
                                "headline": ({"container": best, **modes4k[best]} if best else None),
                                "headline_rule": "the fastest mode whose size is within 0.001 bpp of the reference-format container of the same image",
                                "headline_is_tested_mode": bool(best == IMAGE_4K_HEADLINE), "ac": r4k_ac, **modes4k}
        del big
        legs.free()
        # (informational legs must not cost the line its timed value: a failure in one of them is recorded, not raised)
        for leg_name, leg_fn in (("api_path", lambda: api_path_leg(torch, dev, B, H, W)),
                                 ("api_path_mixed", lambda: api_path_mixed_leg(torch, dev, B)),
                                 ("overlapped_streams", lambda: overlap_leg(torch, dev, sd, rgb, dmode[0])),
                                 ("natural_like", lambda: natural_like_leg(torch, dev, B, H, W, mode)),
                                 ("model_drawn", lambda: model_drawn_leg(torch, dev, B, H, W, mode))):
            try:
                legs_out[leg_name] = leg_fn()
            except Exception as e:
                legs_out[leg_name] = {"skipped": repr(e)[:300]}
                print(f"[bench] leg {leg_name} failed: {e!r}", file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
        try:
            legs_out["roofline_cdf_table"] = table_kernel_roofline(codec, torch)
        except Exception as e:
            legs_out["roofline_cdf_table"] = {"skipped": repr(e)[:300]}

    # whole job: time = MAX over ranks, bytes / pixels = SUM over ranks (the only collectives of the run)
    coll_dev = dev if (world == 1 or args.backend == "nccl") else "cpu"
    agg = shard.aggregate(elapsed, total_bytes, B * H * W, device=coll_dev)
    have_pcie = elapsed_pcie is not None              # the same on every rank (same arguments): the collectives below match
    agg_pcie = shard.aggregate(elapsed_pcie, 0, B * H * W, device=coll_dev) if have_pcie else None
    agg_pcie_serial = shard.aggregate(elapsed_pcie_serial, 0, B * H * W, device=coll_dev) if have_pcie else None
    # per-rank detail (one small all_gather): own time of the timed steps, own pipelined PCIe-inclusive step (0: not measured), physical device
    per = shard.gather_per_rank([elapsed, elapsed_pcie if have_pcie else 0.0, float(shard.device_identity(dev)), float(local_dev),
                                 float(-1 if numa["numa_node"] is None else numa["numa_node"]), float(numa["cpus_bound"])], device=coll_dev)
    idents = [int(p[2]) for p in per]
    per_rows, straggler = shard.per_rank_report([p[0] for p in per], [p[1] for p in per], B * H * W, args.steps, idents, [int(p[3]) for p in per],
                                                numa=[(p[4], p[5]) for p in per])
    n_distinct = shard.distinct_devices(idents)
    if n_distinct < world and not args.allow_shared_gpu:
        # e.g. every rank given the same HIP_VISIBLE_DEVICES: local indices differ from the launcher's view, the silicon does not
        raise SystemExit(f"{world} ranks ran on {n_distinct} distinct GPU(s) (PCI identities {idents}): not a multi-GPU measurement; "
                         "pass --allow-shared-gpu for a rehearsal")
    shared_gpu = shared_gpu or n_distinct < world
    elapsed = agg["elapsed_s"]

    rc = 0
    if rank == 0:
        pix = agg["pixels"]
        value = pix * args.steps / elapsed / 1e6
        flops = 2.0 * MAC_PER_POSITION * positions_per_image(H, W) * B * 2      # rank 0's launches: encode + decode pass
        achieved = flops / (cnn_ms * 1e-3) / 1e12 if cnn_ms > 0 else 0.0
        if world == 8 and B == 32 and (H, W) == (512, 768):
            tag = "; BASELINE.json configs[4] (256 images sharded 32 per GPU)"
        elif B == 24 and mode != MODE_AC and (H, W) == (512, 768):
            tag = "; BASELINE.json configs[2]" + ("" if world == 1 else f" per GPU x {world} GPUs")
        else:
            tag = ""
        out = {
            "metric": "MPix/s encode+decode", "value": round(value, 3), "unit": "MPix/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"{B}x{W}x{H} uniform-noise RGB per GPU, container {args.container} -> {container_out}, seed-1337 weights" + tag,
                       "batch_per_gpu": B, "height": H, "width": W, "container": args.container, "container_written": container_out,
                       "container_is": ("encoder mode xauto<M>: xwide rANS v4 streams, M = what the image's size gives; the encoder picks the image's own count on the device "
                                        "from what its last stage costs -- a pure function of the image (llicti_amd.codec.MODE_RANS_AUTO); container_written = what came out, "
                                        "read from the headers once outside the timed region and handed to the decoder" if (mode & 0x10000) else "as named"),
                       "sharding": f"images/{world}gpu", "backend": args.backend if world > 1 else None},
            "rccl_ranks": rccl_ranks, "ranks": world, "backend": (args.backend if world > 1 else None),
            "distinct_devices": n_distinct, "shared_gpu": bool(shared_gpu),
            "per_rank": per_rows, "straggler_ratio": straggler,
            "bpp": round(agg["bpp"], 4),
        }
        if args.full:
            out.update({
                "n1_companion": n1_companion,
                "efficiency_like_for_like": (round(value / (world * n1_companion["value"]), 4) if n1_companion and n1_companion.get("value") else None),
                "efficiency_is": ("value / (N x n1_companion.value): rank 0 ALONE on its GPU, the same per-GPU batch and container, timed in this very run before the process "
                                  "group formed -- `bench.py --gpus 1` times another batch size (24 against 32 at N = 8)" if world > 1 else None),
                "value_is": "HBM-resident: inputs and containers in HBM when the timed region starts (a PCIe-inclusive rate is "
                            "never `value`).  SURVEY 8(d)'s wording -- H2D of the RGB and D2H of the streams inside -- is value_pcie_inclusive, beside it",
                "value_resident": round(value, 3),
                "value_pcie_inclusive": round(agg_pcie["pixels"] / agg_pcie["elapsed_s"] / 1e6, 3) if have_pcie else None,
                "value_pcie_serial": round(agg_pcie_serial["pixels"] / agg_pcie_serial["elapsed_s"] / 1e6, 3) if have_pcie else None,
                "pcie_inclusive_repeats_mpix_s": pcie_spread, "pcie_pipeline_trace": pcie_trace,
                "pcie_note": "same step with H2D of RGB + D2H of containers (encode) and H2D of containers + D2H of RGB (decode) inside "
                             "the timed region, pinned host buffers, whole container stride copied; value_pcie_inclusive: transfers on their own "
                             "HIP streams, double buffered, overlapped with compute (decode of step k-1 behind encode of step k), steady state = (long run - short run) / extra steps; value_pcie_serial: "
                             "transfer, compute, transfer one after the other",
                "enc_mpix_s": round(B * H * W / t_enc / 1e6, 3), "dec_mpix_s": round(B * H * W / t_dec / 1e6, 3),
                "roofline": {"bound": "mfma", "kernel": "band_params_kernel<0|1|2> (fp32 MFMA 16x16x4)",
                             "achieved": round(achieved, 3), "peak": PEAK_FP32_MATRIX_TFLOPS, "unit": "TFLOP/s",
                             "frac": round(achieved / PEAK_FP32_MATRIX_TFLOPS, 4), "traffic": pmc_traffic("band_params_kernel"),
                             "frac_is": "from HIP events around the launches of one profiled encode + decode of THIS run (llicti_last_timing_detail): the events are "
                                        "release points, so each span holds its launch's write-back and dispatch gap (~40 us of ~700) -- a few percent below frac_rocprof",
                             "frac_rocprof": (lambda r: round(flops / (r["cnn_ms_per_step"] * 1e-3) / 1e12 / PEAK_FP32_MATRIX_TFLOPS, 4) if r and (B, H, W) == (24, 512, 768) else None)(cnn_rocprof()),
                             "rocprof": cnn_rocprof(),
                             "launches": cnn_launches, "kernel_ms_per_step": round(cnn_ms, 3),
                             "call_ms_profiled": round(call_ms, 3),
                             "flop_per_step": flops,
                             # the WHOLE path against the MFMA roof (the step's algorithmic FLOP / the timed step)
                             "whole_path_frac": round(flops / (elapsed / args.steps) / 1e12 / PEAK_FP32_MATRIX_TFLOPS, 4),
                             "cnn_tflops_per_level": {f"level{l}": round(2.0 * MAC_PER_POSITION * level_positions(H, W, l) * B * 2 / (cnn_level_ms[l] * 1e-3) / 1e12, 2)
                                                      for l in range(5) if cnn_level_ms[l] > 0},
                             "kernel_ms": kernel_ms},
                # "the coder itself is integer / latency-bound: report symbols/s" -- the step's coded symbols (3 colour channels of every
                # pixel but the raw DC band) over the entropy coder's own kernels of the profiled encode / decode (HIP events around the launches)
                "coder": (lambda nsym, e, d: {
                    "symbols_per_step": nsym,
                    "encode_gsym_s": round(nsym / ((e.get("rans_encode", 0.0) + e.get("ac", 0.0)) * 1e-3) / 1e9, 3) if (e.get("rans_encode", 0.0) + e.get("ac", 0.0)) > 0 else None,
                    "decode_gsym_s": round(nsym / ((d.get("rans_stage", 0.0) + d.get("rans_tail", 0.0) + d.get("ac", 0.0)) * 1e-3) / 1e9, 3)
                                     if (d.get("rans_stage", 0.0) + d.get("rans_tail", 0.0) + d.get("ac", 0.0)) > 0 else None,
                    "encode_with_pairs_gsym_s": round(nsym / ((e.get("rans_encode", 0.0) + e.get("ac", 0.0) + e.get("cdf_pairs", 0.0)) * 1e-3) / 1e9, 3)
                                                if (e.get("rans_encode", 0.0) + e.get("ac", 0.0) + e.get("cdf_pairs", 0.0)) > 0 else None,
                    "what": "encode: the rANS / range-coder kernel alone (its (c_low, c_high) pairs come from cdf_pairs_kernel: the second figure has both); decode: the "
                            "stage launches + the tail -- the decoder evaluates the mixture CDF inside its symbol search, so this is search + coder"})(
                    3 * (H * W - (H // 32) * (W // 32)) * B, kernel_ms.get("encode", {}), kernel_ms.get("decode", {})),
            })
        if ac_bytes is not None:
            fx, fx_path = _latest_profile_json("bpp_delta_fixtures.json")
            ac_bpp = legs_out["ac_container"]["bpp"]
            out["bpp_delta_vs_reference"] = {
                "timed_container_minus_reference_format_bpp": round(8.0 * (total_bytes - ac_bytes) / (B * H * W), 5),   # rank 0's batch
                "reference_format_container_bpp": ac_bpp,
                "oracle_tables_vs_reference_tables": fx,
                "source": fx_path,
                "note": "reference-format (AC) container: same format, Delta = the table differences of the fixed-arithmetic spec vs the "
                        "reference's PyTorch floats (fixtures). rANS containers: same tables and symbols, about 6 bytes per 64-lane stream (v3), 2.5 - 5 per 256-lane stream (v4) over the ideal "
                        "code length (0.001 bpp = 49 bytes per 768x512 image; the AC container's 45 terminations cost about 25) -- see m_sweep"}
            dbpp = out["bpp_delta_vs_reference"]["timed_container_minus_reference_format_bpp"]
            # + what the build's tables cost against the reference's own PyTorch tables on full-size images of this workload (committed
            #   measurement: tests/golden/ref_ideal_bits.json vs the oracle, profiles/<round>/bpp_delta_fixtures.json "full_size")
            tab = (fx or {}).get("full_size", {}).get("max_abs_delta_bpp")
            if tab is None:
                # the table term is a COMMITTED measurement (it needs the reference's Python, which cannot run on the GPU box): without it
                # the conjunction is undecided, not true
                out["meets_north_star"] = None
                tab = float("nan")
            else:
                tab = abs(float(tab))
                out["meets_north_star"] = bool(value / world >= NORTH_STAR_MPIX_S and abs(dbpp) + tab <= NORTH_STAR_DBPP and (H, W) == (512, 768) and not shared_gpu)
            out["north_star_check"] = {"mpix_s_per_gpu": round(value / world, 3), "min_mpix_s": NORTH_STAR_MPIX_S, "delta_bpp": dbpp,
                                       "tables_vs_reference_tables_full_size_abs_delta_bpp": (None if tab != tab else tab),
                                       "tables_term_is": "a committed measurement (" + str(fx_path) + "), not a per-run one: it needs the reference's own Python",
                                       "max_abs_delta_bpp": NORTH_STAR_DBPP,
                                       "lossless": True, "what": "timed container vs the reference-format container on the same batch (same tables, same symbols); "
                                                                 "decode(encode(x)) == x asserted on a poisoned workspace; image 0 of both containers == CPU oracle bytes (cpu_baseline)"}
        out.update(legs_out)
        rt = legs_out.get("roofline_cdf_table") or {}
        if "bound" in rt:
            # SURVEY 8(d)(ii) beside 8(d)(i) in the `roofline` object itself (the full record stays at roofline_cdf_table)
            out["roofline"]["regime_ii_cdf_table"] = {"bound": rt["bound"], "kernel": rt["kernel"], "frac": rt["frac"], "unit": rt["unit"],
                                                      "hbm_frac": rt["hbm"]["frac"], "hbm_achieved_gbs": rt["hbm"]["achieved"],
                                                      "traffic": rt["traffic"], "full_record": "roofline_cdf_table"}
        nl = legs_out.get("natural_like") or {}
        if "meets_north_star" in out and out["meets_north_star"] is not None and "bpp_delta_budget_image0" in nl:
            # the budget on natural-like content too (tables + container on the full-size fixture image), and the committed row must be about
            # the bytes this GPU wrote
            ok_nl = bool(nl["bpp_delta_budget_image0"] <= NORTH_STAR_DBPP and nl.get("image0_bytes_equal_committed_oracle", False))
            out["north_star_check"]["natural_like_budget_bpp"] = nl["bpp_delta_budget_image0"]
            out["north_star_check"]["natural_like_ok"] = ok_nl
            out["meets_north_star"] = bool(out["meets_north_star"] and ok_nl)
        if args.full and not args.no_cpu_baseline and world == 1:
            cb, bl = cpu_baseline(H, W)
            if cont_ac0 is not None:
                # the same image through the HIP path (reference-format container) must give the oracle's bytes
                got = container_to_bytestream_list(cont_ac0, seg_ac0)
                cb["bitexact_vs_hip"] = bool(got == bl)
                if not cb["bitexact_vs_hip"]:
                    print("[bench] FAIL: HIP container of image 0 differs from the CPU oracle's", file=sys.stderr, flush=True)
                    rc = 3
            if mode != MODE_AC:
                # ... and so must image 0 of the TIMED container (the oracle's restatement of the rANS v3 format)
                from oracle import oracle as orc
                ref_r = orc.encode_image_rans(rgb_h[0], cpu_weights(), mode & 0xFF, ((mode & 0xF00) - 0x100) // 0x200, auto=bool(mode & 0x10000))
                got_r = container_to_bytestream_list(cont[0].cpu().numpy(), seg_h[0])
                cb["timed_container_bitexact_vs_hip"] = bool(got_r == ref_r)
                if not cb["timed_container_bitexact_vs_hip"]:
                    print("[bench] FAIL: timed (rANS) container of image 0 differs from the CPU oracle's", file=sys.stderr, flush=True)
                    rc = 3
            if not args.no_torch_cpu:
                try:
                    cb["torch_cpu"] = cpu_baseline_torch(H, W)
                    if bl is not None:                 # its streams are the oracle's to a few bytes (another erfc, another summation order)
                        n_or = sum(len(x) for row in bl[1:] for x in row)
                        cb["torch_cpu"]["stream_bytes_minus_oracle"] = cb["torch_cpu"]["stream_bytes"] - n_or
                except Exception as e:                 # a baseline, not a gate
                    cb["torch_cpu"] = {"skipped": repr(e)[:200]}
            out["cpu_baseline"] = cb
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()
    return rc


if __name__ == "__main__":
    sys.exit(main() or 0)
