"""The BASELINE.json sizes themselves on the GPU ("no -m gpu test runs any BASELINE size"):

* one training step at each full size - 513^2 B=16+16 bf16 (configs[1]), 769^2 B=8+8 deep stem / OHEM bf16 (configs[3] shape), the same
  with Q=1024 / N=2048 and forced-valid pseudo labels (configs[4] shape: every class has >= Q hard pixels),
  321^2 B=2+2 fp32 (configs[0]) - checked through size-independent properties: finite losses, the supervised loss of a random-init
  network = ln K, every parameter moved, two independent runs agree bit for bit (round 4: ordered reductions);
* the c1 configuration (321^2, B=2, fp32) against the CPU oracle directly: logits and embeddings within the 1e-3 bar of north_star;
* the bf16 throughput path of the whole step against the oracle at 65^2 with the sampler draws injected (the fp32 path has the
  golden traces of test_train_step_gpu.py): supervised and contrastive loss 2e-2, prototypes cosine > 0.97 (mean > 0.99).

Reference: /root/reference/mix_label.py:162-196 (step), generalframeworks/networks/deeplabv3/deeplabv3.py:151-169 (network).
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import dev, rel_err  # noqa: E402


def one_step(workload, dtype, steps=1, **kw):
    import bench
    tr, batch, meta = bench.build(workload, dev(), 0, dtype, "cutmix", "identity", **kw)
    np.random.seed(0)                     # cutmix boxes are drawn on the host with numpy, like the reference
    p0 = tr.flat_p.clone()
    outs = [tr.step(*batch) for _ in range(steps)]
    torch.cuda.synchronize()
    res = dict(losses=[{k: float(v) for k, v in o.items() if k != "pseudo"} for o in outs], moved=(tr.flat_p != p0).float().mean().item(),
               probe=tr.flat_p[:: 4099].clone().cpu(), protos=tr.prototypes.clone().cpu(), finite=bool(torch.isfinite(tr.flat_p).all()), K=meta["K"])
    del tr, batch
    torch.cuda.empty_cache()
    return res


@pytest.mark.parametrize("workload,dtype,kw", [("c2", "bf16", {}), ("c4", "bf16", {}), ("c5", "bf16", dict(forced_valid=True)),
                                               ("c2", "f32", dict(size=321, batch=2))],
                         ids=["c2_513_B16_bf16", "c4_769_B8_stem_ohem_bf16", "c5_769_B8_Q1024_N2048_forced_valid_bf16", "c1_321_B2_fp32"])
def test_full_size_step_properties(workload, dtype, kw):
    a = one_step(workload, dtype, **kw)
    b = one_step(workload, dtype, **kw)
    la, lb = a["losses"][0], b["losses"][0]
    print(workload, dtype, la)
    assert all(math.isfinite(v) for v in la.values()) and a["finite"]
    # random-init network: soft-max is near uniform, CE = ln K (OHEM keeps the hardest pixels: a little above)
    assert abs(la["sup"] - math.log(a["K"])) < (0.15 if workload == "c2" else 0.4), la
    assert la["contrast"] > 0
    assert a["moved"] > 0.99                                     # SGD reached every parameter
    # run-to-run: identical seeds and draws, and since round 4 every reduction of the step is ordered - the two runs agree BIT FOR BIT at the
    # full sizes too (until round 3: 2e-3 on the losses, 2e-2 on weights and prototypes - the order of fp32 atomic adds)
    for k in la:
        assert la[k] == lb[k] or (math.isnan(la[k]) and math.isnan(lb[k])), (k, la[k], lb[k])
    assert torch.equal(a["probe"], b["probe"]) and torch.equal(a["protos"], b["protos"])


def test_forced_valid_variant_feeds_the_unlabeled_half():
    """SURVEY 8(d) forced-valid (used for c5 and extra.c2_forced_valid of bench.py): the unsupervised loss is live."""
    a = one_step("c2", "bf16", size=129, batch=4, forced_valid=True)
    la = a["losses"][0]
    assert la["unsup"] > 0.5 and la["contrast"] > 0 and a["finite"], la


def test_c1_config_logits_vs_oracle_fp32():
    """BASELINE configs[0] geometry (321x321, B=2, fp32, tv-R101, K=21): the HIP network against the CPU oracle on the same
    seeded weights (bn3 gains x0.25: the conditioning of a trained network, see test_network_gpu.py) - north_star's 1e-3."""
    from css_amd.networks import resnet
    from css_amd.networks.deeplabv3.deeplabv3 import DeepLabv3Plus_with_rep
    from oracle import css_oracle as O
    K, S, B, seed, gain = 21, 321, 2, 11, 0.25
    sd = O.init_state("tv", K, 256, seed, gain)
    net = DeepLabv3Plus_with_rep(resnet.resnet101_tv(), dilate_scale=8, num_classes=K, output_dim=256)
    net.load_state_dict(sd, strict=True)
    net = net.to(dev()).train()
    x = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(seed))
    with torch.no_grad():
        po, ro = O.deeplab_forward(sd, x, "tv", True, K, 256)
        pred, rep = net(x.to(dev()))
    e_p, e_r = rel_err(pred.cpu(), po), rel_err(rep.cpu(), ro)
    print(f"c1 321^2 fp32 vs oracle: logits {e_p:.2e} embeddings {e_r:.2e}")
    assert pred.shape == po.shape and e_p < 1e-3 and e_r < 1e-3


def _step_vs_oracle(S, B, dtype, Q, N, seed, blocks, weak=0.0, gain=0.25, floor_runs=0):
    """One MixTrainer.step on the HIP path against oracle.train_step_mix (mix_label.py:162-196) on the same seeded inputs and weights
    (``gain`` 0.25: bn3 gains x0.25, the conditioning of a trained network; 1.0: undamped), the oracle's sampler draws injected.
    ``weak``: the valid-mask threshold of mix_label.py:176 (0.7 in the reference's configs and in bench.py: with these weights about a third of
    the unlabeled pixels pass it; 0.0: every unlabeled pixel is valid).  Returns (hip result, oracle result, trainer, oracle state) and, with
    ``floor_runs`` > 0, a fifth item: the same oracle step re-evaluated with 1-ulp relative perturbations of the images (same injected draws) -
    what two correct fp32 implementations of this step differ by."""
    from css_amd.networks import resnet
    from css_amd.networks.ddp_model import Model_mix
    from css_amd.train_step import MixTrainer
    from oracle import css_oracle as O
    K = 21
    cfg = {"Dataset": {"crop_size": (S, S), "scale_size": (1.0, 1.0), "mix_mode": "none", "device_aug": "identity"}}
    g = torch.Generator().manual_seed(seed)
    l_img, u_img = torch.randn(B, 3, S, S, generator=g), torch.randn(B, 3, S, S, generator=g)
    cell = -(-S // blocks)
    l_lab = torch.randint(0, K, (B, blocks, blocks), generator=g).repeat_interleave(cell, 1).repeat_interleave(cell, 2)[:, :S, :S].clone()
    l_lab[:, : cell // 2, : cell] = -1                        # some ignored pixels, like the reference's 255 -> -1 border
    args = dict(lr=1e-3, temp_model=0.5, strong_threshold=0.8, weak_threshold=weak, un_threshold=0.97, num_queries=Q, num_negatives=N)
    st = O.MixState("tv", K, 256, seed, gain)
    rec = {}
    torch.manual_seed(0)
    np.random.seed(0)
    ro = O.train_step_mix(st, l_img, l_lab, u_img, record=rec, **args)
    floors = []
    for i in range(floor_runs):
        gp = torch.Generator().manual_seed(1000 + i)
        st_i = O.MixState("tv", K, 256, seed, gain)
        rec_i = {}
        r_i = O.train_step_mix(st_i, l_img * (1 + 1e-7 * torch.randn(l_img.shape, generator=gp)), l_lab,
                               u_img * (1 + 1e-7 * torch.randn(u_img.shape, generator=gp)), injected=dict(rec), record=rec_i, **args)
        assert rec_i["present"] == rec["present"]            # (same classes present: the injected draws mean the same thing)
        floors.append((r_i, st_i))
    m = Model_mix(resnet.resnet101_tv(), num_classes=K, output_dim=256, config=cfg, temp=0.5)
    sd = O.init_state("tv", K, 256, seed, gain)
    m.model.load_state_dict(sd)
    m.ema_model.load_state_dict(sd)
    m = m.to(dev()).train().set_compute_dtype(dtype)
    tr = MixTrainer(m, K, lr=1e-3, total_iter=100, num_queries=Q, num_negatives=N, strong_threshold=0.8, weak_threshold=weak, un_threshold=0.97)
    # the class lists the draws index into depend on the hard flags (own-class probability < 0.8): where a pixel near the threshold
    # changes sides the injected indices are taken modulo the list lengths by the kernel (css_contrast_resolve)
    r = tr.step(l_img.to(dev()), l_lab.to(dev()), u_img.to(dev()), _injected=dict(anchor=rec["anchor"], negative=rec["negative"]))
    torch.cuda.synchronize()
    return (r, ro, tr, st, floors) if floor_runs else (r, ro, tr, st)


@pytest.mark.parametrize("weak", [0.0, 0.7], ids=["every_unlabeled_pixel_valid", "weak_threshold_0.7"])
def test_c1_full_step_vs_oracle_fp32(weak):
    """BASELINE configs[0] as a STEP: 321x321, B = 2 + 2, fp32, tv-R101, K = 21, Q = 256, N = 512 - teacher x2, student
    forward / backward x2, the three losses, the prototype EMA, SGD + EMA teacher - against oracle.train_step_mix with injected draws:
    ALL THREE losses 1e-3 (the unsupervised loss was asserted 1000x looser than measured), prototypes 1e-3, pseudo labels
    < 0.5 % mismatching, the updated student weights on a probe.  Second case: the reference's and bench.py's weak threshold 0.7
    (mix_label.py:176), so the valid-mask branch ``u_logits_cls >= weak_thr`` meets the oracle at size with both sides populated."""
    r, ro, tr, st = _step_vs_oracle(321, 2, torch.float32, 256, 512, 11, 10, weak=weak)
    for key in ("sup", "unsup", "contrast"):
        a, b = float(r[key]), float(ro[key])
        print(f"c1 step fp32 weak={weak} {key}: hip {a:.6f} oracle {b:.6f} rel {abs(a - b) / max(1.0, abs(b)):.2e}")
    for key in ("sup", "contrast"):
        a, b = float(r[key]), float(ro[key])
        assert abs(a - b) < 1e-3 * max(1.0, abs(b)), (key, a, b)
    a, b = float(r["unsup"]), float(ro["unsup"])             # a mean over the few pixels above the 0.97 confidence threshold
    assert (math.isnan(a) and math.isnan(b)) or abs(a - b) < 1e-3 * max(1.0, abs(b)), (a, b)
    e = ((tr.prototypes.cpu() - st.prototypes).abs().max() / st.prototypes.abs().max()).item()
    mism = (r["pseudo"].cpu() != ro["pseudo"]).float().mean().item()
    print(f"c1 step fp32: prototypes rel {e:.2e}, pseudo labels mismatching {mism:.2e}")
    assert e < 1e-3 and mism < 5e-3, (e, mism)
    # the optimizer's result: updated student weights, and the UPDATE itself (lr x nesterov(gradient + wd x weight)) as a direction -
    # a wrong gradient scale or a missed layer shows in the cosine, ReLU-flip noise of two fp32 forwards (test_network_gpu.py) does not
    from oracle import css_oracle as O
    w0 = O.init_state("tv", 21, 256, 11, 0.25)
    names = [n for n in st.pnames if n.endswith("conv3.weight") or n.endswith("conv2.weight") or n.startswith("classifier")
             or n.startswith("representation") or n.startswith("ASPP")][:: 3]
    sdh = tr.model.model.state_dict()
    worst_w, worst_c = 0.0, 1.0
    for n in names:
        wh, wo = sdh[n].detach().cpu().double(), st.student[n].detach().double()
        worst_w = max(worst_w, rel_err(wh, wo))
        worst_c = min(worst_c, torch.nn.functional.cosine_similarity((wh - w0[n].double()).flatten(), (wo - w0[n].double()).flatten(), dim=0).item())
    print(f"c1 step fp32: updated student weights over {len(names)} probed layers: worst rel {worst_w:.2e}, worst update cosine {worst_c:.6f}")
    assert worst_w < 1e-3 and worst_c > 0.995, (worst_w, worst_c)


def _bf16_step_checks(r, ro, tr, st, tag):
    for key in ("sup", "contrast"):
        a, b = float(r[key]), float(ro[key])
        print(f"{tag} bf16 {key}: hip {a:.5f} oracle {b:.5f}")
        assert abs(a - b) < 2e-2 * max(1.0, abs(b)), (key, a, b)
    pa, pb = tr.prototypes.cpu().double(), st.prototypes.double()
    present = pb.abs().sum(1) > 0
    cos = torch.nn.functional.cosine_similarity(pa[present], pb[present], dim=1)
    print(f"{tag} bf16 prototypes: cosine over present classes: min", float(cos.min()), "mean", float(cos.mean()))
    # measured on MI355X at 65^2: min 0.986 (a class with few valid pixels: the mean of a handful of bf16-path embeddings)
    assert present.any() and float(cos.min()) > 0.97 and float(cos.mean()) > 0.99
    mism = (r["pseudo"].cpu() != ro["pseudo"]).float().mean().item()
    print(f"{tag} bf16 pseudo labels mismatching: {mism:.2e}")
    assert mism < 2e-2, mism


def test_bf16_step_vs_oracle_with_injected_draws():
    """The bf16 throughput path of MixTrainer.step against the fp32 CPU oracle at 65x65 (well-conditioned weights, the oracle's
    sampler draws injected): bf16 activations through ~110 batch-stat BN layers - losses within 2e-2, prototype cosines > 0.97 / 0.99 mean."""
    _bf16_step_checks(*_step_vs_oracle(65, 2, torch.bfloat16, 64, 128, 7, 5), "65^2 B=2+2")


@pytest.mark.parametrize("weak", [0.0, 0.7], ids=["every_unlabeled_pixel_valid", "weak_threshold_0.7"])
def test_bf16_step_vs_oracle_129_b4(weak):
    """The same at 129x129, B = 4 + 4, Q = 256, N = 512: here the BN / loss / contrast kernels of the bench dtype
    run multi-tile launches (M = 8 x 17^2 ... 8 x 65^2 rows per layer, two statistics groups of 4 images) against an oracle, not
    only against properties.  Also at the reference's weak threshold 0.7.  This is the largest size at which the bench
    dtype meets the ORACLE; at 513^2 / 769^2 the bf16 step is covered by properties and bit-reproducibility (test_full_size_step_properties)."""
    _bf16_step_checks(*_step_vs_oracle(129, 4, torch.bfloat16, 256, 512, 13, 6, weak=weak), f"129^2 B=4+4 weak={weak}")


def test_undamped_step_vs_oracle_65_fp32():
    """One whole step with UNDAMPED weights (bn3 gains 1.0: activations grow through the 33 residual blocks, the conditioning of a fresh random
    network rather than a trained one) at 65x65, fp32, weak threshold 0.7, against the oracle - judged like test_network_gpu.py judges the
    undamped networks: against max(1e-3, 2 x floor), the floor being what the ORACLE ITSELF moves by under 1-ulp relative perturbations of
    its input images (three draws, same injected sampler draws) - i.e. what two correct fp32 implementations of this step differ by."""
    r, ro, tr, st, floors = _step_vs_oracle(65, 2, torch.float32, 64, 128, 7, 5, weak=0.7, gain=1.0, floor_runs=3)
    rel = lambda a, b: abs(a - b) / max(1.0, abs(b))
    for key in ("sup", "unsup", "contrast"):
        a, b = float(r[key]), float(ro[key])
        if math.isnan(b):
            assert math.isnan(a), (key, a, b)
            continue
        fl = max(rel(float(ri[key]), b) for ri, _ in floors)
        bound = max(1e-3, 2 * fl)
        print(f"undamped 65^2 step fp32 {key}: hip {a:.6f} oracle {b:.6f} rel {rel(a, b):.2e}; oracle's own 1-ulp floor {fl:.2e}; bound {bound:.2e}")
        assert rel(a, b) < bound, (key, a, b, fl)
    pn = st.prototypes.abs().max()
    e = ((tr.prototypes.cpu() - st.prototypes).abs().max() / pn).item()
    fl = max(((si.prototypes - st.prototypes).abs().max() / pn).item() for _, si in floors)
    mism = (r["pseudo"].cpu() != ro["pseudo"]).float().mean().item()
    fl_m = max((ri["pseudo"] != ro["pseudo"]).float().mean().item() for ri, _ in floors)
    print(f"undamped 65^2 step fp32: prototypes rel {e:.2e} (floor {fl:.2e}), pseudo labels mismatching {mism:.2e} (floor {fl_m:.2e})")
    assert e < max(1e-3, 2 * fl) and mism < max(5e-3, 2 * fl_m), (e, fl, mism, fl_m)


def test_bench_dump_outputs_are_the_last_timed_step_and_reproducible(tmp_path):
    """bench.py --dump-outputs: two fresh runs with the same arguments write the same outputs bit for bit (every input is seeded); the
    second runs without the per-kernel profiling step that follows the timed region, so equality also shows the dump precedes it."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    runs = []
    for tag, extra_env in (("a", {}), ("b", {"CSS_BENCH_NOPROF": "1"})):
        d = tmp_path / tag
        env = dict(os.environ, **extra_env)
        env.pop("WORLD_SIZE", None)
        env.pop("RANK", None)
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "3", "--warmup", "1", "--size", "65", "--batch", "2",
                            "--no-extra", "--no-cpu-baseline", "--dump-outputs", str(d)], env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        assert json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])["steps"] == 3
        runs.append({f[:-4]: np.load(d / f) for f in os.listdir(d)})
    a, b = runs
    assert sorted(a) == ["contrast", "prototypes", "pseudo", "student_params", "sup", "teacher_params", "total", "unsup"]
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), k
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert all(np.isfinite(a[k]).all() for k in ("prototypes", "student_params", "teacher_params"))
