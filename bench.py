#!/usr/bin/env python3
"""Throughput of the CSS mix_label training step on MI355X.

    python bench.py --gpus N --steps K --warmup W          (defaults: N = 1, W = 20 - SURVEY 8(d) - and K = 20: ~6 s of steps)

N > 1 with WORLD_SIZE unset: this process starts N fresh children of itself (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* in their
environment, one per GPU) BEFORE it touches the GPU, relays rank 0's line and exits non-zero if any child fails - the counterpart of
the reference's own ``mp.spawn`` (/root/reference/mix_label.py:265).  Under ``python -m torch.distributed.run`` (WORLD_SIZE set) it is
one rank of that job.

A "step" = one iteration of mix_label.train (teacher fwd on labeled+unlabeled, student fwd+bwd on labeled+augmented unlabeled,
CE + confidence-weighted CE + prototype contrastive loss, fused SGD+EMA; /root/reference/mix_label.py:162-196) over B labeled + B
unlabeled synthetic crops per GPU.  Default workload c2 = BASELINE.json configs[1]: VOC-shaped 513x513, torchvision-shaped ResNet-101
DeepLabv3+, B=16, bf16.  Weak scaling: every rank owns its own B+B crops; SyncBN statistics, prototype sums and the flat gradient are
the only exchanges (RCCL).  Rank 0 prints ONE JSON line; at N=1 it also carries
  * ``extra.c4``: 5 steps (after 3 warm-up) of the Cityscapes-shaped 769x769 workload (BASELINE configs[3] shape on one GPU),
  * ``extra.c5``: 5 steps (after 3) of c4 with Q=1024, N=2048, forced-valid (BASELINE configs[4] shape),
  * ``extra.c2_forced_valid``: 5 steps (after 3) of c2 with every unlabeled pixel valid (SURVEY 8d "forced-valid": worst-case contrastive load),
  * ``extra.c2_aug_pil``: 5 steps (after 3) of c2 with the reference's in-step augmentation on the device inside the timed step,
  * ``extra.c2_cross_trainer`` / ``extra.c2_ori_trainer``: 3 steps (after 3) of the two other entry scripts' train bodies at the c2 shapes,
  * ``cpu_baseline``: the CPU oracle timed on the host cores.

``--dump-outputs DIR`` writes what the last timed step of the headline leg computed (rank 0) as DIR/<name>.npy, float32 / float64:
the dict the step returns (losses, pseudo labels) and the state it updated in place (prototypes, student and teacher weights); an output
of more than DUMP_MAX_ELEMS elements is written as a fixed, seeded sample of its elements.  Every input of a leg is seeded, so two builds
run with the same arguments can be compared output for output.
"""
import argparse
import contextlib
import ctypes
import json
import os
import random
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

FWD_FLOP_513_TV = 541.7e9          # forward FLOPs / image, tv-R101, 513^2, K=21
FWD_FLOP_769_STEM = 1239.1e9       # deep-stem R101, 769^2, K=19
PEAK_BF16 = 2.5e15                 # MI355X dense bf16 MFMA (MI355X_MICROARCH.md)
PEAK_F32 = 157.3e12
PEAK_HBM = 8.0e12                  # HBM3E spec (MI355X_MICROARCH.md; 6.29 TB/s measured by a float4 copy)

KINDS = ((0, "conv_fwd_other"), (1, "conv_dgrad_other"), (2, "conv_wgrad_other"), (3, "contrast_gather"), (4, "similarity"),
         (5, "igemm256_fwd"), (6, "igemm256_dgrad"), (7, "wgrad256"), (8, "bn_apply"), (9, "bn_bwd_apply"), (10, "bn_bwd_reduce"),
         (11, "sgd_ema"), (12, "conv1x1_short_k_fwd"), (13, "conv_ws_flops"), (14, "conv_ws_bytes"), (15, "igemm256_bytes"))
WORKLOADS = {
    # name: (K, S, B, backbone, sup, Q, N, BASELINE configs index)
    "c2": (21, 513, 16, "tv", "ce", 256, 512, 1),
    "c4": (19, 769, 8, "stem", "ohem", 256, 512, 3),
    "c5": (19, 769, 8, "stem", "ohem", 1024, 2048, 4),
}


# ---- N > 1 without a launcher: start the ranks ourselves -------------------------------------------------------------------------
def source_sha256():
    """Digest of the product sources this line was measured on (scripts/source_hash.py; checked by tests/test_host_cpu.py)."""
    try:
        import importlib.util
        spec = importlib.util.spec_from_file_location("source_hash", os.path.join(ROOT, "scripts", "source_hash.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod.source_hash(ROOT)
    except Exception:
        return None


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


RC_RENDEZVOUS = 75                 # a child could not bind / reach the rendezvous port: the launcher retries on a new port


def launch_children(n, argv, timeout_s=1800.0, attempts=3):
    """Start n fresh python processes of this file (never a re-exec of a process that touched the GPU), wait for all, relay rank 0's
    stdout (children inherit it: only rank 0 prints) and return non-zero if any of them failed.  Bounded: after ``timeout_s`` (a rank
    stuck in a collective while every process stays alive) the children are terminated, then killed after a grace period, and the
    result is 124.  The port is picked by binding and closing a socket, so another job can take it before the children bind: a child
    that fails at the rendezvous exits with RC_RENDEZVOUS and the launch is repeated on a new port (``attempts`` times)."""
    def stop(ps):
        for q in ps:                  # exactly the PIDs we started
            q.terminate()
        t_end = time.time() + 10.0
        for q in ps:
            try:
                q.wait(max(0.1, t_end - time.time()))
            except subprocess.TimeoutExpired:
                q.kill()              # a rank inside RCCL may ignore SIGTERM
                q.wait()

    rc = 1
    for _ in range(attempts):
        port = free_port()
        procs = []
        for r in range(n):
            env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
            env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env))
        rc = 0
        alive = list(procs)
        t_end = time.time() + timeout_s
        while alive:
            for p in list(alive):
                r = p.poll()
                if r is None:
                    continue
                alive.remove(p)
                if r != 0 and rc == 0:
                    rc = r if r > 0 else 1
                    stop(alive)       # a dead rank leaves the others blocked in a collective
            if alive and time.time() > t_end:
                print(f"bench.py: {len(alive)} rank(s) still running after {timeout_s:.0f} s - stopping them", file=sys.stderr)
                stop(alive)
                return 124
            time.sleep(0.05)
        if rc != RC_RENDEZVOUS:
            return rc
        print("bench.py: rendezvous failed, retrying on a new port", file=sys.stderr)
    return rc


# ---- workload ------------------------------------------------------------------------------------------------------------------------
def synth_batch(B, S, K, seed, dev):
    """images N(0,1); labels piecewise-constant 32x32 blocks uniform over K classes, 5 % of blocks = -1.
    Also returns block labels for the unlabeled crops (no ignore blocks): used by the forced-valid variant only."""
    g = torch.Generator().manual_seed(seed)
    l_img = torch.randn(B, 3, S, S, generator=g)
    u_img = torch.randn(B, 3, S, S, generator=g)
    nb = (S + 31) // 32
    blk = torch.randint(0, K, (B, nb, nb), generator=g)
    blk[torch.rand(B, nb, nb, generator=g) < 0.05] = -1
    l_lab = blk.repeat_interleave(32, 1).repeat_interleave(32, 2)[:, :S, :S].contiguous()
    ublk = torch.randint(0, K, (B, nb, nb), generator=g)
    u_blk = ublk.repeat_interleave(32, 1).repeat_interleave(32, 2)[:, :S, :S].contiguous()
    return l_img.to(dev), l_lab.to(dev), u_img.to(dev), u_blk.to(dev)


def make_trainer_class(forced_valid, script="mix"):
    from css_amd.train_step import CrossTrainer, MixTrainer, OriTrainer
    if script != "mix":          # the two other entry scripts of the reference (cross_label.py:153-200, ori_pseudo.py:149-189)
        return CrossTrainer if script == "cross" else OriTrainer
    if not forced_valid:
        return MixTrainer

    class ForcedValidTrainer(MixTrainer):
        """SURVEY 8(d) "forced-valid": the teacher still runs (no work is skipped), but the pseudo labels that reach the losses are
        the synthetic block labels with confidence 1 and every valid pixel counts as hard - so the unlabeled half feeds the
        unsupervised loss, all K classes have >= Q hard pixels and the contrastive pool is at its largest (mask_all = 1)."""
        forced_labels = None

        def _student_outputs(self, l_img, u_img):
            pred_l, pred_u, (u_lab, u_lc), _, rep_all, small = super()._student_outputs(l_img, u_img)
            lab = self.forced_labels
            conf = torch.ones_like(u_lc)
            return pred_l, pred_u, (lab, conf), (lab, conf), rep_all, small

        def _hard_flags(self, rep_nhwc, cls, pred_small):
            return (cls >= 0).to(torch.uint8)

    return ForcedValidTrainer


BN_GAMMA_NOTE = ("BN gamma ~ U(0.25, 0.75), beta ~ N(0, 0.1) - SURVEY 8(d) says gamma ~ U(0.5, 1.5): the narrower draw keeps the residual stream of the "
                 "random-init network O(1) through 33 blocks, so the supervised loss starts at ln K (tests/test_full_size_gpu.py asserts it); the "
                 "kernels, their launch shapes and their work are identical for any gamma")


def build(workload, dev, rank, dtype="bf16", mix="cutmix", aug="identity", forced_valid=False, size=None, batch=None, script="mix"):
    """-> (trainer, (l_img, l_lab, u_img), meta) for one rank: seeded non-degenerate weights (Kaiming convs from the
    constructor, BN gamma ~ U(.25,.75), beta ~ N(0,.1)), synthetic crops of the workload's shape."""
    from css_amd.networks import resnet
    from css_amd.networks.ddp_model import Model_cross, Model_mix, Model_ori_pseudo
    K, S, B, backbone, sup, Q, N, cfg_idx = WORKLOADS[workload]
    S, B = size or S, batch or B
    torch.manual_seed(3407)
    np.random.seed(3407 + rank)           # the host draws of the step (cutmix boxes; the in-step augmentation also uses random)
    random.seed(3407 + rank)
    cfg = {"Dataset": {"crop_size": (S, S), "scale_size": (0.5, 1.5) if aug == "pil" else (1.0, 1.0), "mix_mode": mix, "device_aug": aug}}
    bb = resnet.resnet101_tv(zero_init_residual=False) if backbone == "tv" else resnet.resnet101(zero_init_residual=False)
    with contextlib.redirect_stdout(sys.stderr):     # the constructor prints like the reference's; stdout carries the ONE JSON line only
        if script == "mix":
            model = Model_mix(bb, num_classes=K, output_dim=256, config=cfg, temp=0.5)
        elif script == "cross":
            model = Model_cross(bb, num_classes=K, output_dim=256, config=cfg, temp=0.5)
        else:
            model = Model_ori_pseudo(bb, num_classes=K, output_dim=256, config=cfg)
    g = torch.Generator().manual_seed(3407)
    with torch.no_grad():
        for mod in model.model.modules():
            if mod.__class__.__name__ == "HipBatchNorm2d":
                mod.weight.copy_(torch.rand(mod.weight.shape, generator=g) * 0.5 + 0.25)
                mod.bias.copy_(torch.randn(mod.bias.shape, generator=g) * 0.1)
        model.ema_model.load_state_dict(model.model.state_dict())
    model = model.to(dev).train().set_compute_dtype(torch.bfloat16 if dtype == "bf16" else torch.float32)
    tr = make_trainer_class(forced_valid, script)(model, K, lr=6.4e-3, total_iter=80000, num_queries=Q, num_negatives=N, strong_threshold=0.8,
                                          weak_threshold=0.7, un_threshold=0.97, sup=sup, ohem_min_kept=50000 * B)
    l_img, l_lab, u_img, u_blk = synth_batch(B, S, K, 3407 + rank, dev)
    if forced_valid:
        tr.forced_labels = u_blk
    meta = dict(K=K, S=S, B=B, backbone=backbone, sup=sup, Q=Q, N=N, cfg_idx=cfg_idx,
                fwd_flop=(FWD_FLOP_513_TV * (S / 513.0) ** 2 if backbone == "tv" else FWD_FLOP_769_STEM * (S / 769.0) ** 2))
    return tr, (l_img, l_lab, u_img), meta


def read_prof():
    from css_amd import _lib
    prof = {}
    for kind, name in KINDS:
        ms, n, w = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        _lib.lib().css_prof_read(kind, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(w))
        prof[name] = (ms.value, n.value, w.value)
    return prof


DUMP_MAX_ELEMS = 1 << 22          # --dump-outputs: larger outputs are sampled (16 MB each in float32; at most three are: < 64 MB in all)


def dump_outputs(tr, out, d):
    """--dump-outputs: write the step's returned dict and the state it updated in place (prototypes, flat student / teacher weights) as
    d/<name>.npy.  Floating outputs as float32 (float64 stays float64), integer ones (pseudo labels) as float32, exact below 2^24; an output
    of more than DUMP_MAX_ELEMS elements as the flat sample at positions drawn once from a fixed seed (the same for every build)."""
    arrays = dict(out, prototypes=tr.prototypes, student_params=tr.flat_p, teacher_params=tr.flat_ema)
    host, positions = {}, {}
    for name, t in arrays.items():
        t = t.detach()
        n = t.numel()
        if n > DUMP_MAX_ELEMS:
            if n not in positions:
                positions[n] = torch.randperm(n, generator=torch.Generator().manual_seed(0))[:DUMP_MAX_ELEMS].sort().values.to(t.device)
            t = t.reshape(-1)[positions[n]]
        if not t.is_floating_point():
            assert t.numel() == 0 or int(t.abs().max()) < 2 ** 24, name
        host[name] = (t.double() if t.dtype == torch.float64 else t.float()).cpu().numpy()
    total = sum(a.nbytes for a in host.values())
    assert total <= 64 << 20, total
    os.makedirs(d, exist_ok=True)
    for name, a in host.items():
        np.save(os.path.join(d, name + ".npy"), a)
    print(f"bench.py: {len(host)} outputs of the last timed step ({total / 2 ** 20:.1f} MB) -> {d}", file=sys.stderr)


def timed_run(tr, batch, steps, warmup, world, dev, profile=True, dump_dir=None):
    """W untimed steps, then EXACTLY K timed steps bracketed by barrier + synchronize on both sides; MAX over ranks.
    Per-kernel HIP-event bracketing (roofline leg; ~2.8 us per event pair on the launch stream, ~2.6 ms per step) runs in ONE EXTRA
    step after the timed region (r02 verdict, weak 14: the timed steps are all in one mode).  ``dump_dir``: the outputs of the last
    timed step are written there (dump_outputs) between the timed region and that extra step, which would overwrite them."""
    from css_amd import _lib

    def sync():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(warmup):
        tr.step(*batch)
    _lib.lib().css_prof_reset()
    sync()
    t0 = time.perf_counter()
    for i in range(steps):
        out = tr.step(*batch)
    sync()
    dt = time.perf_counter() - t0
    if dump_dir:
        dump_outputs(tr, out, dump_dir)
    if profile and not os.environ.get("CSS_BENCH_NOPROF"):
        _lib.lib().css_prof_enable(1)
        tr.step(*batch)
        sync()
        _lib.lib().css_prof_enable(0)
    if hasattr(tr, "finish"):
        tr.finish()
    if world > 1:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t)
    prof = read_prof()
    _lib.lib().css_prof_reset()
    return dt, out, prof


def pmc_traffic(workload):
    """HBM bytes per launch of the dominant convolution kernels, REPLAYED from the committed rocprofv3 PMC passes of this workload (separate
    FETCH_SIZE / WRITE_SIZE runs of this same command, FETCH_SIZE doubled per the gfx950 correction of MI355X_MICROARCH.md) -
    PMC counters cannot be collected from inside the run that prints the line.  (None, None) when no pass exists for the workload."""
    import csv
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", f"r*_pmc_hbm_traffic_{workload}.csv")))
    if not files and workload == "c2":
        files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_hbm_traffic.csv")))
    if not files:
        return None, None
    rd = wr = n = 0.0
    for r in csv.DictReader(open(files[-1])):
        if "conv_igemm_pp" in r["kernel"] or "conv_igemm_p8" in r["kernel"]:
            k = float(r["launches"])
            rd += float(r["read_MB_per_launch_corrected_x2"]) * k
            wr += float(r["write_MB_per_launch"]) * k
            n += k
    if not n:
        return None, None
    return round((rd + wr) / n * 1e6), f"profiles/{os.path.basename(files[-1])} (replayed)"


def rooflines(prof, dtype, workload, step_conv_flops=None):
    """step_conv_flops: the algorithmic conv FLOPs of one step (8 B F for mix / cross, 7 B F for ori_pseudo - SURVEY 8d)."""
    def tot(*names):
        return tuple(sum(prof[n][i] for n in names) for i in range(3))
    peak = PEAK_BF16 if dtype == "bf16" else PEAK_F32
    # the dominant kernel = the persistent 256x256-tile kernels alone: kinds 5 + 6 minus the conv_ws_kernel launches filed there too (13)
    ig_ms, ig_n, ig_fl = (a - b for a, b in zip(tot("igemm256_fwd", "igemm256_dgrad"), prof["conv_ws_flops"]))
    ach = ig_fl / (ig_ms * 1e-3) if ig_ms > 0 else 0.0
    traffic, src = pmc_traffic(workload)
    roof = {"bound": "mfma", "kernel": "conv_igemm_p8_kernel (+ conv_igemm_pp_kernel for the shapes with < 3 K steps of 64): the persistent 256x256-tile "
                                       "implicit-GEMM convolution on the 8-phase K loop, every forward + dgrad launch of one step after the timed region "
                                       "(the short-K 1x1 class runs on conv_ws_kernel: see kernels.conv_ws_kernel)",
            "achieved": round(ach / 1e12, 2), "peak": peak / 1e12, "unit": "TFLOP/s", "frac": round(ach / peak, 4),
            "traffic": traffic, "traffic_source": src, "launches_per_step": ig_n, "avg_launch_us": round(ig_ms * 1e3 / max(ig_n, 1), 2),
            "alg_flops_per_launch": ig_fl / max(ig_n, 1),
            # algorithmic HBM bytes of the same launches (source + weights + output once each, + addend and mask): `traffic` is read against this
            "alg_bytes_per_launch": round(prof["igemm256_bytes"][2] / max(prof["igemm256_bytes"][1], 1)),
            "traffic_over_alg_bytes": (round(traffic / (prof["igemm256_bytes"][2] / max(prof["igemm256_bytes"][1], 1)), 3)
                                       if traffic and prof["igemm256_bytes"][2] > 0 else None)}
    # SURVEY 8(d)'s own definition of the MFMA fraction: (8 B F / t_conv) / peak with t_conv = EVERY convolution kernel of the step (forward,
    # data gradient, weight gradient: persistent, weight-stationary, leftover, narrow and stem launches alike), HIP events of the profiled step
    t_conv = tot("conv_fwd_other", "igemm256_fwd", "conv_dgrad_other", "igemm256_dgrad", "conv_wgrad_other", "wgrad256")[0]
    if step_conv_flops and t_conv > 0:
        roof["mfma_frac_all_conv"] = round(step_conv_flops / (t_conv * 1e-3) / peak, 4)
        roof["all_conv_ms_per_step"] = round(t_conv, 3)
        roof["mfma_frac_all_conv_is"] = "(8 B F / sum of all conv kernel time of the step) / peak - SURVEY 8(d); `frac` is the dominant kernel alone"
    # (keys name the kernels that run today: the big-tile class = conv_igemm_p8_kernel + conv_ws_kernel launches, forward and dgrad)
    mfma_groups = {"conv_igemm_p8_and_ws_kernels": tot("igemm256_fwd", "igemm256_dgrad"), "conv_wgrad_p8_kernel": prof["wgrad256"],
                   "conv_fwd_all_kernels": tot("conv_fwd_other", "igemm256_fwd"), "conv_dgrad_all_kernels": tot("conv_dgrad_other", "igemm256_dgrad"),
                   "conv_wgrad_all_kernels": tot("conv_wgrad_other", "wgrad256")}
    hbm_groups = {k: prof[k] for k in ("bn_apply", "bn_bwd_apply", "bn_bwd_reduce", "sgd_ema", "conv1x1_short_k_fwd", "contrast_gather", "similarity")}
    mfma_groups["conv_ws_kernel"] = prof["conv_ws_flops"]
    hbm_groups["conv_ws_kernel_hbm"] = prof["conv_ws_bytes"]
    kernels = {}
    for k, v in mfma_groups.items():
        rate = v[2] / max(v[0] * 1e-3, 1e-12)
        kernels[k] = {"bound": "mfma", "ms_per_step": round(v[0], 3), "launches_per_step": v[1], "achieved_TFLOPs": round(rate / 1e12, 2),
                      "frac": round(rate / peak, 4)}
    for k, v in hbm_groups.items():
        rate = v[2] / max(v[0] * 1e-3, 1e-12)
        kernels[k] = {"bound": "hbm", "ms_per_step": round(v[0], 3), "launches_per_step": v[1], "achieved_GBs": round(rate / 1e9, 1),
                      "peak_GBs": PEAK_HBM / 1e9, "frac": round(rate / PEAK_HBM, 4)}
    return roof, kernels


def cpu_baseline(budget_s=150.0):
    """The oracle (CPU restatement of the reference path, kind 'port') on BASELINE configs[0] (321x321, B=2+2, fp32, tv-R101,
    Q=256, N=512, the GPU step's thresholds), protocol of BASELINE.md section 4: 1 warm-up step + 3 timed steps at N = all host
    threads, then N = 8 for comparison with the build container - bounded: once ``budget_s`` of wall time is spent no further step
    is started (at least one timed step always runs; the sample string says what was done)."""
    import numpy as np
    from oracle import css_oracle as O
    K, S, B = 21, 321, 2
    g = torch.Generator().manual_seed(3407)
    l_img, u_img = torch.randn(B, 3, S, S, generator=g), torch.randn(B, 3, S, S, generator=g)
    blk = torch.randint(0, K, (B, 11, 11), generator=g)
    l_lab = blk.repeat_interleave(32, 1).repeat_interleave(32, 2)[:, :S, :S].contiguous()
    args = dict(lr=6.4e-3, temp_model=0.5, strong_threshold=0.8, weak_threshold=0.7, un_threshold=0.97, num_queries=256, num_negatives=512)
    t_start = time.time()
    n_all = torch.get_num_threads()

    st = O.MixState("tv", K, 256, 3407)
    torch.manual_seed(0)
    np.random.seed(0)

    def run(threads, max_timed):
        torch.set_num_threads(threads)
        ts = []
        while len(ts) < max_timed and (not ts or time.time() - t_start + ts[-1] < budget_s):
            t0 = time.time()
            O.train_step_mix(st, l_img, l_lab, u_img, **args)
            ts.append(time.time() - t0)
        return ts

    torch.set_num_threads(n_all)
    O.train_step_mix(st, l_img, l_lab, u_img, **args)                     # warm-up step (allocator, oneDNN primitives), all threads
    # the 8-thread sample comes FIRST (one timed step), so that it is never dropped for lack of budget (r02 verdict, weak 12)
    t8 = run(8, 1) if n_all > 8 else None
    ts = run(n_all, 3)                                                    # at least one timed step, then as many as the budget allows
    res = {"value": round(2 * B * len(ts) / sum(ts), 4), "unit": "images/s", "cores": n_all, "kind": "port",
           "sample": f"1 warm-up + {len(ts)} timed steps of mix_label.train semantics at BASELINE configs[0] (321x321, B=2+2, fp32, tv-R101, "
                     f"Q=256, N=512, weak_threshold=0.7), {sum(ts) / len(ts):.1f} s per step"}
    if t8 is not None:
        res["at_8_threads"] = {"value": round(2 * B * len(t8) / sum(t8), 4), "cores": 8,
                               "sample": f"{len(t8)} timed step after the all-thread warm-up step, {sum(t8) / len(t8):.1f} s per step"}
    else:
        res["at_8_threads"] = "same run (the host has 8 threads or fewer)"
    torch.set_num_threads(n_all)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=20, help="SURVEY 8(d): 20 steps before timing (prototype EMA branch active)")
    ap.add_argument("--batch", type=int, default=None, help="crops per GPU of each kind (default: the workload's)")
    ap.add_argument("--size", type=int, default=None, help="crop size (default: the workload's)")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--mix", default="cutmix")
    ap.add_argument("--aug", default="identity", choices=["identity", "pil"])
    ap.add_argument("--workload", default="c2", choices=list(WORKLOADS),
                    help="c2: VOC-shaped 513^2 tv-R101 B=16 (default, the headline metric); c4: Cityscapes-shaped 769^2 deep-stem R101 "
                         "K=19 OHEM B=8; c5: c4 with Q=1024, N=2048, forced-valid")
    ap.add_argument("--forced-valid", action="store_true", help="SURVEY 8(d) forced-valid variant (always on for c5)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extra", action="store_true", help="skip the extra.c4 / extra.c2_forced_valid legs")
    ap.add_argument("--cpu-budget", type=float, default=150.0)
    ap.add_argument("--timeout", type=float, default=0.0, help="self-launcher (--gpus N without WORLD_SIZE): stop the ranks after this many "
                                                               "seconds (default: 600 + 30 per step)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step of the headline leg computed as DIR/<name>.npy (rank 0; < 64 MB in all)")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    # ---- launch decision: BEFORE anything touches the GPU ----
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_children(a.gpus, sys.argv[1:], a.timeout if a.timeout > 0 else 600.0 + 30.0 * (a.steps + a.warmup)))

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        sys.exit(f"bench.py: --gpus {a.gpus} but WORLD_SIZE={world}")
    # stdout carries ONE JSON line.  Libraries write there too (RCCL prints its version banner to stdout when a communicator is
    # created): keep the real stdout aside and point file descriptor 1 at stderr for the duration of the run.
    sys.stdout.flush()
    real_stdout = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)
    # launcher self-test (tests/test_host_cpu.py): rendezvous + one collective over gloo on CPU, no GPU, no model
    if os.environ.get("CSS_BENCH_LAUNCH_TEST"):
        if os.environ["CSS_BENCH_LAUNCH_TEST"] == f"fail{rank}":
            sys.exit(3)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        t = torch.tensor([float(rank + 1)])
        dist.all_reduce(t)
        if rank == 0:
            print(json.dumps({"launch_test": True, "n_gpus": world, "sum": float(t)}), file=real_stdout, flush=True)
        dist.destroy_process_group()
        return
    # CSS_BENCH_SHARE_GPU=1: every rank on cuda:0 with gloo collectives - the N > 1 code path on a one-GPU box (tests only)
    share = os.environ.get("CSS_BENCH_SHARE_GPU") == "1"
    if share:
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    # CSS_FORCE_COLLECTIVES=1 on one GPU: a 1-rank RCCL group with every data-parallel exchange switched on (ops.collectives_on) -
    # measures what the collective calls of a step cost before any wire time
    forced = world == 1 and os.environ.get("CSS_FORCE_COLLECTIVES") == "1"
    if world > 1 or forced:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29581")
        try:
            if share:
                dist.init_process_group("gloo", rank=rank, world_size=world)
            else:
                dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        except (RuntimeError, OSError, dist.DistNetworkError) as e:        # the port went to someone else between free_port() and here
            print(f"bench.py rank {rank}: rendezvous failed: {e}", file=sys.stderr)
            sys.exit(RC_RENDEZVOUS)

    def run_leg(workload, steps, warmup, forced_valid, profile=True, size=None, batch=None, aug=None, script="mix", dump_dir=None):
        tr, batch_t, meta = build(workload, dev, rank, a.dtype, a.mix, aug or a.aug, forced_valid, size, batch, script)
        dt, out, prof = timed_run(tr, batch_t, steps, warmup, world, dev, profile, dump_dir)
        roof, kernels = rooflines(prof, a.dtype, workload, (7 if script == "ori" else 8) * meta["B"] * meta["fwd_flop"])
        losses = {k: round(float(v), 4) for k, v in out.items() if k != "pseudo"}
        del tr, batch_t
        torch.cuda.empty_cache()
        return dt, losses, roof, kernels, meta

    rccl = None
    if dist.is_initialized():
        ones = torch.ones(1, device=dev)
        dist.all_reduce(ones)                    # what the communicator itself says about the number of ranks
        rccl = {"backend": dist.get_backend(), "world_size": dist.get_world_size(), "nranks_allreduce_check": int(ones.item()),
                "forced_one_rank_group": bool(forced)}
        if dist.get_backend() == "nccl":
            try:
                rccl["version"] = ".".join(str(v) for v in torch.cuda.nccl.version())
            except Exception:
                pass
    fv = a.forced_valid or a.workload == "c5"
    dt, losses, roof, kernels, meta = run_leg(a.workload, a.steps, a.warmup, fv, True, a.size, a.batch,
                                              dump_dir=a.dump_outputs if rank == 0 else None)
    S, B, K = meta["S"], meta["B"], meta["K"]
    if rank == 0:
        shape = "VOC-shaped" if meta["backbone"] == "tv" else "Cityscapes-shaped"
        net = "tv-ResNet-101" if meta["backbone"] == "tv" else "deep-stem ResNet-101"
        res = {
            "metric": f"training images/sec at {S}x{S} R101-DeepLabv3+ (mix_label step, labeled+unlabeled crops consumed)",
            "value": round(2 * B * world * a.steps / dt, 3), "unit": "images/s", "n_gpus": dist.get_world_size() if dist.is_initialized() else 1, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": round(dt / a.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": a.dtype, "data": "synthetic",
            "config": {"workload": (f"BASELINE configs[{meta['cfg_idx']}]{' shape' if a.workload != 'c2' else ''}: {shape} mix_label step, {net} "
                                    f"DeepLabv3+, {S}x{S}, B={B}+{B} per GPU, K={K}, sup={meta['sup']}, Q={meta['Q']}, N={meta['N']}, "
                                    f"mix_mode={a.mix}, device_aug={a.aug}" + (", forced-valid pseudo labels" if fv else "")),
                       "global_batch": 2 * B * world, "parallelism": f"dp{world}", "weights": BN_GAMMA_NOTE},
            "roofline": roof, "kernels": kernels,
            "step_alg_tflops": round(8 * B * meta["fwd_flop"] / (dt / a.steps) / 1e12, 2),
            "losses": losses, "source_sha256": source_sha256(),
        }
        if rccl:
            res["rccl"] = rccl
    if world == 1 and not a.no_extra and a.workload == "c2" and a.size is None and a.batch is None:
        extra = {}
        n4, w4 = 5, 3
        d4, l4, r4, k4, m4 = run_leg("c4", n4, w4, False)
        extra["c4"] = {"workload": "BASELINE configs[3] shape on one GPU: Cityscapes-shaped, deep-stem ResNet-101, 769x769, B=8+8, K=19, OHEM",
                       "value": round(2 * m4["B"] * n4 / d4, 3), "unit": "images/s", "ms_per_step": round(d4 / n4 * 1e3, 3), "steps": n4, "warmup": w4,
                       "roofline": {k: r4[k] for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "traffic_source", "avg_launch_us",
                                                       "alg_bytes_per_launch", "traffic_over_alg_bytes", "mfma_frac_all_conv", "all_conv_ms_per_step") if k in r4},
                       "step_alg_tflops": round(8 * m4["B"] * m4["fwd_flop"] / (d4 / n4) / 1e12, 2), "losses": l4}
        n5, w5 = 5, 3
        d5, l5, r5, k5, m5 = run_leg("c5", n5, w5, True)
        extra["c5"] = {"workload": "BASELINE configs[4] shape on one GPU: c4 with Q=1024, N=2048 and SURVEY 8(d) forced-valid pseudo labels (the "
                                   "stress case of the contrastive gather)",
                       "value": round(2 * m5["B"] * n5 / d5, 3), "unit": "images/s", "ms_per_step": round(d5 / n5 * 1e3, 3), "steps": n5, "warmup": w5,
                       "contrast_gather": k5["contrast_gather"], "losses": l5}
        n2, w2 = 5, 3
        d2, l2, r2, k2, m2 = run_leg("c2", n2, w2, True, profile=False)
        extra["c2_forced_valid"] = {"what": "c2 with SURVEY 8(d) forced-valid pseudo labels (unlabeled half feeds the unsupervised loss and the "
                                            "contrastive pool: losses.unsup != 0)",
                                    "value": round(2 * m2["B"] * n2 / d2, 3), "unit": "images/s", "ms_per_step": round(d2 / n2 * 1e3, 3), "steps": n2,
                                    "warmup": w2, "losses": l2}
        # the in-step augmentation of the reference INSIDE the timed step (ddp_model.py:121-137): random rescale 0.5-1.5, crop,
        # colour jitter, blur, flip on the device (csrc/aug.hip), cutmix - the headline line times the identity stand-in
        d6, l6, _, _, m6 = run_leg("c2", n2, w2, False, profile=False, aug="pil")
        extra["c2_aug_pil"] = {"what": "c2 with device_aug='pil': the reference's in-step augmentation (VOC.py:126-196,325-352) on the device inside the "
                                       "timed step", "value": round(2 * m6["B"] * n2 / d6, 3), "unit": "images/s", "ms_per_step": round(d6 / n2 * 1e3, 3),
                               "steps": n2, "warmup": w2, "losses": l6}
        # the two other entry scripts (VERDICT r04 missing 4): cross_label.py:153-200 (8 B F per step) and ori_pseudo.py:149-189 (7 B F per step)
        for script, ref in (("cross", "cross_label.py:153-200, warm-up branch"), ("ori", "ori_pseudo.py:149-189")):
            ns, wsu = 3, 3
            ds, ls, _, _, ms_ = run_leg("c2", ns, wsu, False, profile=False, script=script)
            extra[f"c2_{script}_trainer"] = {"what": f"c2 shapes through {'CrossTrainer' if script == 'cross' else 'OriTrainer'} ({ref})",
                                             "value": round(2 * ms_["B"] * ns / ds, 3), "unit": "images/s", "ms_per_step": round(ds / ns * 1e3, 3),
                                             "steps": ns, "warmup": wsu, "losses": ls,
                                             "step_alg_tflops": round((7 if script == "ori" else 8) * ms_["B"] * ms_["fwd_flop"] / (ds / ns) / 1e12, 2)}
        res["extra"] = extra
    if rank == 0:
        if world == 1 and not a.no_cpu_baseline:
            res["cpu_baseline"] = cpu_baseline(a.cpu_budget)
        print(json.dumps(res), file=real_stdout, flush=True)
    if world > 1 or forced:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
