#!/usr/bin/env python3
"""masked-forward-passes/sec benchmark (BASELINE.json metric).

    python bench.py --gpus 1 --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W
    python bench.py --gpus N ...        (no launcher: this process starts the N ranks itself and touches no GPU)

One "step" = one pass of the hot path over the workload of BASELINE configs[2]
("ResNet-101, 512 masks/image x 128 images, 1 MI355X"): per image, K0 stages its 512 masked
copies, the network scores them, 512 scores stay on the device.  With N GPUs every rank runs its
own 128 images (weak scaling; N=8 is BASELINE configs[3], 1024 images) and ONE RCCL all-gather of
the per-mask scores closes the step.  Inputs (images, label map, mask-vectors, weights) are
resident in HBM before the timed region.  Rank 0 prints one JSON line.

A plain run sets up, warms up, times the K steps and prints the line.  Everything else the line can
carry -- the per-kernel profile step and `roofline`, the CPU baseline and the parity of the engine's
scores against it (`cpu_baseline`, `parity`, `score_max_abs_delta`, `argmax_agree`) -- is measured
only under --full; a plain run reports those fields as null.  --dump-outputs DIR writes what the last
timed step computed (DIR/scores.npy, DIR/preds.npy; float32) for output-for-output comparison of two
builds: the inputs are seeded, so the same arguments give the same inputs on every run.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_F16_MFMA_TFLOPS = 2500.0   # MI355X dense fp16/bf16 MFMA, /opt/skills/guides/MI355X_MICROARCH.md
F16X3_CEILING_TFLOPS = PEAK_F16_MFMA_TFLOPS / 3.0   # three MFMA products per algorithmic product
PEAK_F32_MFMA_TFLOPS = 157.3    # exact-f32 MFMA (v_mfma_f32_16x16x4_f32), same guide: the pipe the reference's own arithmetic type would run on
DUMP_MAX_BYTES = 64 << 20       # --dump-outputs: all files together
DUMP_SAMPLE_SEED = 20240601     # --dump-outputs: the fixed sample of an output too large to write whole


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--arch", default="resnet101")
    ap.add_argument("--images", type=int, default=128, help="images per GPU per step")
    ap.add_argument("--masks", type=int, default=512, help="masks per image")
    ap.add_argument("--images-per-forward", type=int, default=0,
                    help="forward batch = this x masks (0 = --forward-batch decides)")
    ap.add_argument("--forward-batch", type=int, default=0,
                    help="slots per forward batch; the mask rows of consecutive images are packed into such batches.  0 = the "
                         "largest batch <= 2400 that cuts the 14x14 maps into WHOLE rounds of tiles over the 256 CUs "
                         "(engine.whole_round_batch: 2340; at 2048 the last round of the 3x3 and reducing 1x1 layers is 1/8 full)")
    ap.add_argument("--stem", choices=("table", "conv"), default=None,
                    help="how the masks are staged (MaskedForwardEngine(stem=...)): 'table' = the stem by superposition (the engine's default on the "
                         "ImageNet ResNets), 'conv' = K0 + the MFMA stem conv + max pool (rounds 1-3)")
    ap.add_argument("--cpu-masks", type=int, default=16, help="masks of the CPU baseline sample (--full only; 0 = skip)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline figure does not need: one profiled step after the timed region (`roofline`) "
                         "and, at one rank, the CPU baseline and the engine-vs-CPU parity on its sample")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed as DIR/<name>.npy (float32; %d MB at most in all, "
                         "a fixed seeded sample of larger outputs)" % (DUMP_MAX_BYTES >> 20))
    ap.add_argument("--force-dist", action="store_true",
                    help="initialise torch.distributed (RCCL) and run the all-gather even with one rank (rehearsal of the N>1 path)")
    ap.add_argument("--stub-step", action="store_true",
                    help="TEST HOOK, not a measurement: no GPU and no engine -- gloo on the CPU and a step that fills the rank's block of "
                         "scores with a function of the flat (image, mask) index; exercises the launcher, the rendezvous, the barrier / "
                         "max-over-ranks timing and the all-gather, and prints a line whose `data` says \"stub\" (tests/test_bench_launcher.py)")
    args = ap.parse_args(argv)
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


def pmc_traffic(arch, batch):
    """HBM bytes of the conv kernels per forward batch from the committed rocprofv3 PMC passes (FETCH_SIZE / WRITE_SIZE
    cannot be read from inside the process) -> (bytes per forward batch, file name); (None, None) unless a profile of this arch
    exists.  A file taken at another forward batch is scaled by the batch ratio (activation bytes are proportional to the batch,
    the 0.18 GB of weights are not: the source string says so)."""
    import glob
    best = None
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc_traffic*.json")), reverse=True):
        with open(path) as fh:
            j = json.load(fh)
        if arch != j.get("arch", "resnet101"):
            continue
        if best is None or (j.get("forward_batch") == batch and best[0].get("forward_batch") != batch):
            best = (j, path)
    if best is None:
        return None, None
    j, path = best
    total = j["write_bytes_per_batch"] + j["fetch_corrected_bytes_per_batch_guide_x2"]
    name = os.path.relpath(path, ROOT)
    if j["forward_batch"] != batch:
        return total * batch / j["forward_batch"], "%s (measured at forward batch %d, scaled by %d/%d)" % (name, j["forward_batch"], batch, j["forward_batch"])
    return total, name


def _cpu_model():
    try:
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def _cpu_inputs(n_masks, seg_block=16):
    from network_interpretation_imagenet_amd import synth
    img = synth.make_images(1, kind="noise")[0]
    seg = synth.grid_segments(block=seg_block)
    return img, seg, synth.random_onoff(n_masks, int(seg.max()) + 1)


def _cpu_loop(arch, n_masks, threads, label=0):
    """Reference-style loop (oracle/scorer.py: batch-1 fp32 forward per mask, mask built per superpixel)
    -> (fwd/s, s, score f32[n_masks], pred i32[n_masks])."""
    from network_interpretation_imagenet_amd import synth
    from oracle import scorer
    torch.set_num_threads(threads)
    sd = synth.make_state_dict(arch)
    img, seg, onoff = _cpu_inputs(n_masks)
    x = scorer.to_tensor_normalize(img)
    scorer.score_masks_reference_loop(sd, arch, x, seg, onoff[:1], label)    # warm the thread pool
    t0 = time.perf_counter()
    score, pred = scorer.score_masks_reference_loop(sd, arch, x, seg, onoff, label)
    dt = time.perf_counter() - t0
    return n_masks / dt, dt, score, pred


def cpu_baseline(arch, n_masks, eng=None):
    """the reference-style CPU loop on this box's host cores, bounded samples: the benched arch
    (`value`, comparable with the GPU line) on all threads, and BASELINE cfg-1 exactly (ResNet-18, 1 image, 64 masks)
    on all threads and on ONE thread; CPU model and thread count stated.  With `eng` (the benched engine, same arch and the
    same synthetic weights) the SAME masks are scored on the GPU as well: -> (cpu_baseline object, parity object) where parity
    is the second half of BASELINE.json's metric ("score max|d| vs ref"): max |score_gpu - score_cpu| over the sample and
    whether every argmax agrees (generate_gp_training_data_imagenet.py:246-248, bayesian_active_learning_imagenet.py:196-198)."""
    import numpy as np
    all_threads = torch.get_num_threads()
    label, parity = 0, None
    if eng is not None:
        img, seg, onoff = _cpu_inputs(n_masks)
        label, _p = eng.predict(img)                    # the reference scores the class the unmasked image is predicted as
        # the sample goes through the staging the TIMED step used (eng.stem: the stem table by default -- 16 rows alone would fall under
        # the engine's 256-row threshold and take K0 + the MFMA stem), and through the other staging as a second field
        _o, g_score, g_pred = eng.score_masks(img, seg, onoff, label, stem=eng.stem)
        other = "conv" if eng.stem == "table" else None
        if other:
            _o, o_score, o_pred = eng.score_masks(img, seg, onoff, label, stem=other)
    # the host's honest best for this loop (SURVEY 8d "all cores and also = 1"): a batch-1 conv does not scale to a
    # hundred threads, so the same sample (same masks, same batch-1 fp32 loop) runs at 1, 8, 32 and all threads and the BEST is `value`
    by_threads = {}
    for th in sorted({1, min(8, all_threads), min(32, all_threads), all_threads}):
        r = _cpu_loop(arch, n_masks, th, label)
        by_threads[th] = r
    best_th = max(by_threads, key=lambda th: by_threads[th][0])
    v, dt, c_score, c_pred = by_threads[best_th]
    if eng is not None:
        delta = lambda s: float(np.abs(s.astype(np.float64) - c_score.astype(np.float64)).max())
        parity = {"score_max_abs_delta": delta(g_score),
                  "argmax_agree": bool((g_pred == c_pred).all()), "tolerance": 1e-4,
                  "staging": "%s (the staging of the timed step: %s)" % (eng.stem, "mpx_stem_table_build + mpx_stem_table_apply" if eng.stem == "table"
                                                                          else "mpx_mask_apply_normalize + the MFMA stem"),
                  "sample": "%s, 1 noise image x %d masks (the cpu_baseline sample), label = unmasked argmax %d: engine.score_masks(stem=%r) "
                            "against the batch-1 fp32 torch-CPU loop (oracle/scorer.py)" % (arch, n_masks, label, eng.stem),
                  "score_range": [float(c_score.min()), float(c_score.max())]}
        if other:
            parity["other_staging"] = {"staging": "conv (mpx_mask_apply_normalize + the MFMA stem: what a call under %d rows per image takes)" % eng.stem_table_min_rows,
                                       "score_max_abs_delta": delta(o_score), "argmax_agree": bool((o_pred == c_pred).all()),
                                       "max_abs_delta_between_stagings": float(np.abs(o_score.astype(np.float64) - g_score.astype(np.float64)).max())}
    c1_all, dt_all, _s, _p = _cpu_loop("resnet18", 64, all_threads)
    c1_one, dt_one, _s, _p = _cpu_loop("resnet18", 16, 1)
    c1_8, dt_8, _s, _p = _cpu_loop("resnet18", 64, min(8, all_threads))
    torch.set_num_threads(all_threads)
    from oracle import resnet_ref
    gf18 = resnet_ref.flops_per_forward("resnet18") / 1e9
    base = {"value": v, "unit": "masked-forward-passes/s", "cores": best_th, "kind": "port",
            "sample": "%s, 1 image x %d masks, batch-1 fp32 torch-CPU loop (%.1f s), best of %s threads" % (arch, n_masks, dt, sorted(by_threads)),
            "by_threads": {str(th): {"value": r[0], "seconds": r[1],
                                     "score_max_abs_delta_vs_best": float(np.abs(r[2].astype(np.float64) - c_score.astype(np.float64)).max())}
                           for th, r in sorted(by_threads.items())},
            "cpu_model": _cpu_model(), "logical_cpus": os.cpu_count(),
            "cfg1_resnet18_1x64": {"all_threads": {"value": c1_all, "threads": all_threads, "seconds": dt_all, "gflops": c1_all * gf18},
                                   "one_thread": {"value": c1_one, "threads": 1, "seconds": dt_one, "gflops": c1_one * gf18,
                                                  "sample": "16 of the 64 masks"},
                                   "eight_threads": {"value": c1_8, "threads": min(8, all_threads), "seconds": dt_8, "gflops": c1_8 * gf18}}}
    return base, parity


def dump_outputs(dirname, arrays):
    """--dump-outputs: {name: 1-D tensor or array} -> DIR/<name>.npy in float32.  Outputs that together exceed DUMP_MAX_BYTES are cut to
    the same fixed, seeded sample of positions (all of the same length), whose flat indices go to DIR/sample_index.npy (float64)."""
    import numpy as np
    arrays = {k: np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v).reshape(-1).astype(np.float32) for k, v in arrays.items()}
    n = max(a.size for a in arrays.values())
    keep = (DUMP_MAX_BYTES - 4096) // (4 * len(arrays) + 8)        # 4 kB for the .npy headers
    os.makedirs(dirname, exist_ok=True)
    if n > keep:
        assert all(a.size == n for a in arrays.values()), "a sampled dump needs outputs of one length"
        idx = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(n, keep, replace=False))
        arrays = {k: a[idx] for k, a in arrays.items()}
        np.save(os.path.join(dirname, "sample_index.npy"), idx.astype(np.float64))
    for k, a in arrays.items():
        np.save(os.path.join(dirname, k + ".npy"), a)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_ranks(n, argv, stub=False, grace_s=None):
    """`python bench.py --gpus N` without a launcher: start N fresh child processes of this script, one per GPU, with
    RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT set (what torch.distributed.run would export), wait for them, and
    return a non-zero code if any failed.  The others are then sent SIGTERM and, if they have not exited `grace_s` seconds later (a rank
    blocked in a collective or a kernel does not see the signal), SIGKILL; whatever ends this function -- an exception, Ctrl-C -- every
    child is reaped on the way out.  Rank 0's JSON line reaches stdout because the children inherit it.  This parent never touches
    a GPU: it only COMPILES the library when its stamp is stale (hipcc; the ranks then find a fresh stamp and load it themselves) --
    it does not dlopen it, so no HIP runtime is initialised here and nothing is exec'ed from a process that has one.  With the stub step
    (`--stub-step`, the CPU test hook) nothing is compiled at all."""
    if grace_s is None:
        grace_s = float(os.environ.get("MPX_BENCH_KILL_GRACE_S", "10"))
    if not stub:
        import __graft_entry__ as g
        g.compile_only()
    env = dict(os.environ)
    env.setdefault("MASTER_ADDR", "127.0.0.1")
    env.setdefault("MASTER_PORT", str(_free_port()))
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env["WORLD_SIZE"] = str(n)
    env["LOCAL_WORLD_SIZE"] = str(n)
    procs = []
    rc = 0
    try:
        for r in range(n):
            e = dict(env)
            e["RANK"] = e["LOCAL_RANK"] = str(r)
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=e))
        pending = set(range(n))
        kill_at = None
        while pending:
            for r in sorted(pending):
                code = procs[r].poll()
                if code is None:
                    continue
                pending.discard(r)
                if code != 0 and rc == 0:
                    rc = code if code > 0 else 1
                    sys.stderr.write("bench.py: rank %d exited with %d; stopping the other ranks\n" % (r, code))
                    for q in pending:
                        procs[q].terminate()
                    kill_at = time.monotonic() + grace_s
            if pending and kill_at is not None and time.monotonic() >= kill_at:
                for q in pending:
                    sys.stderr.write("bench.py: rank %d ignored SIGTERM for %.0f s; killing it\n" % (q, grace_s))
                    procs[q].kill()
                kill_at = float("inf")
            if pending:
                time.sleep(0.05)
    finally:
        for p in procs:                     # an exception or Ctrl-C in the loop above must not leave ranks behind
            if p.poll() is None:
                p.kill()
            try:
                p.wait(timeout=30)
            except subprocess.TimeoutExpired:
                pass
    return rc


def timed_steps(step, fence, steps, warmup, use_dist, device, record_events=True):
    """The bench contract's timed region: W untimed steps, then EXACTLY K steps bracketed by fence() (barrier +
    synchronize) on both sides, wall time MAX over ranks -> (seconds, GPU-side ms between two HIP events or None, last step's result)."""
    for _ in range(warmup):
        step()
    fence()
    ev0 = ev1 = None
    if record_events:
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    if ev0 is not None:
        ev0.record()
    out = None
    for _ in range(steps):
        out = step()
    if ev1 is not None:
        ev1.record()
    fence()
    dt = time.perf_counter() - t0
    gpu_ms = ev0.elapsed_time(ev1) if ev0 is not None else None
    if use_dist:
        t = torch.tensor([dt], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    return dt, gpu_ms, out


def stub_main(args, rank, world):
    """--stub-step (test hook): the launcher / rendezvous / timing / all-gather skeleton of main() on the CPU under gloo."""
    from network_interpretation_imagenet_amd import shard
    if os.environ.get("MPX_BENCH_STUB_FAIL_RANK") == str(rank):      # the launcher test's failing rank: the others must not outlive it
        raise SystemExit(3)
    if os.environ.get("MPX_BENCH_STUB_DEAF_RANK") == str(rank):      # ... and a rank that ignores SIGTERM (as one blocked in a collective does)
        import signal
        signal.signal(signal.SIGTERM, signal.SIG_IGN)
        time.sleep(600)
    use_dist = world > 1 or args.force_dist
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        dist.init_process_group("gloo", rank=rank, world_size=world)
    n_img, n_mask = args.images, args.masks
    total = world * n_img * n_mask
    lo, hi = shard.block(total, rank, world)
    w = torch.arange(lo, hi, dtype=torch.float64)

    def step():
        local = (torch.sin(w * 0.37) * 0.5 + 0.5).to(torch.float32)
        return shard.all_gather_blocks(local, total) if use_dist else local

    def fence():
        if use_dist:
            dist.barrier()

    dt, _ms, out = timed_steps(step, fence, args.steps, args.warmup, use_dist, torch.device("cpu"), record_events=False)
    want = (torch.sin(torch.arange(total, dtype=torch.float64) * 0.37) * 0.5 + 0.5).to(torch.float32)
    assert out.numel() == total and bool((out == want).all()), "stub: gathered scores differ from the single-process values"
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, {"scores": out})
    if rank == 0:
        print(json.dumps({"metric": "masked-forward-passes/sec (stub)", "value": total * args.steps / dt, "unit": "masked-forward-passes/s",
                          "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3,
                          "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "none",
                          "data": "stub (TEST HOOK: no GPU, no engine, gloo on the CPU -- not a measurement)",
                          "config": {"workload": "stub step, %d x %d indices per rank (x%d ranks)" % (n_img, n_mask, world)}}))
    if use_dist:
        dist.destroy_process_group()


def main(argv=None):
    args = parse(argv)
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # started without a launcher: this process becomes one (it never initialises a GPU)
        raise SystemExit(launch_ranks(args.gpus, sys.argv[1:] if argv is None else argv, stub=args.stub_step))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d (start it as `python bench.py --gpus N`, or under torch.distributed.run with "
                         "--nproc-per-node N)" % (args.gpus, world))
    if args.stub_step:
        return stub_main(args, rank, world)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    use_dist = world > 1 or args.force_dist
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)     # "nccl" is RCCL on ROCm

    import __graft_entry__ as g
    if local_rank == 0:     # one builder per node; the other ranks only load the finished library
        g.build()
    if use_dist:
        dist.barrier()
    from network_interpretation_imagenet_amd import _lib, shard, synth
    _lib.load()
    from network_interpretation_imagenet_amd.engine import MaskedForwardEngine

    from network_interpretation_imagenet_amd.engine import whole_round_batch
    n_img, n_mask = args.images, args.masks
    if args.images_per_forward:
        batch = args.images_per_forward * n_mask
    else:
        batch = args.forward_batch or whole_round_batch(2400, num_cus=torch.cuda.get_device_properties(local_rank).multi_processor_count)
    batch = min(batch, n_img * n_mask)
    batches_per_step = n_img * n_mask / batch          # forward batches per step (the last one of a step may be partial)
    sd = synth.make_state_dict(args.arch)
    eng = MaskedForwardEngine(args.arch, max_batch=batch, device=local_rank, stem=args.stem).load_state_dict(sd)
    # synthetic inputs, resident in HBM: this rank's images, the shared 14x14-block label map (S=196),
    # per-image Bernoulli(0.4) mask-vectors, labels = unmasked argmax (the reference's correctness gate)
    imgs = torch.from_numpy(synth.make_images(n_img, seed=1234 + rank, kind="noise")).to(dev)
    seg = torch.from_numpy(synth.grid_segments()).to(dev)
    onoff = torch.from_numpy(synth.random_onoff(n_img * n_mask, 196, seed=4321 + rank)).view(n_img, n_mask, 196).to(dev)
    ones = torch.ones(1, 196, dtype=torch.uint8, device=dev)
    labels = []
    for i0 in range(0, n_img, batch):          # unmasked forwards, one slot per image
        nb = min(batch, n_img - i0)
        for j in range(nb):
            eng.stage_masks(imgs[i0 + j], seg, ones, j)
        _s, p = eng.forward(nb, torch.zeros(nb, dtype=torch.int32, device=dev))
        labels.append(p)
    labels = torch.cat(labels)
    label_rows = labels.view(n_img, 1).expand(n_img, n_mask).contiguous()
    scores = torch.empty(n_img, n_mask, dtype=torch.float32, device=dev)      # outputs pre-allocated: the step allocates nothing
    preds = torch.empty(n_img, n_mask, dtype=torch.int32, device=dev)
    total = world * n_img * n_mask

    img_list = list(imgs)
    onoff_list = list(onoff)
    label_flat = label_rows.view(-1)

    def step():
        # the product entry (MaskedForwardEngine.score_packed): the mask rows of consecutive images share forward batches of
        # `batch` slots -- K0 per image, then the network, for every (image, mask) of this rank; allocates and synchronises nothing
        eng.score_packed(img_list, seg, onoff_list, label_flat, scores.view(-1), preds.view(-1))
        if use_dist:
            return shard.all_gather_blocks(scores.view(-1), total)
        return scores.view(-1)

    def fence():
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    # the timed region: exactly K steps, nothing but the step inside (no per-kernel events, no allocation); ONE pair of
    # HIP events on the launch stream brackets it for the GPU-side time
    dt, gpu_ms_timed, out = timed_steps(step, fence, args.steps, args.warmup, use_dist, dev)
    assert out.numel() == total and bool(torch.isfinite(out).all())
    if args.dump_outputs:
        # what a caller of the step receives: the (gathered) scores and the argmax of every (image, mask), before anything else runs
        all_preds = shard.all_gather_blocks(preds.view(-1).to(torch.float32), total) if use_dist else preds.view(-1)
        if rank == 0:
            dump_outputs(args.dump_outputs, {"scores": out, "preds": all_preds})
    # --full: per-kernel durations: ONE more step of the same work after the timed region, every launch bracketed by HIP events
    # on its stream (engine profile pool)
    prof = {"ms": {}, "launches": {}}
    batches_profiled = forwards_profiled = 0
    if rank == 0 and args.full:
        step_imgs = n_img
        rows = step_imgs * n_mask
        eng.profile(True)
        eng.score_packed(img_list[:step_imgs], seg, onoff_list[:step_imgs], label_flat[:rows], scores.view(-1)[:rows], preds.view(-1)[:rows])
        eng.profile(False)
        prof = eng.collect_profile()
        batches_profiled = rows / batch
        forwards_profiled = -(-rows // batch)
        torch.cuda.synchronize()
    if use_dist:
        dist.barrier()

    if rank == 0:
        value = total * args.steps / dt
        cfg_name = {("resnet101", 512, 128): "BASELINE configs[2]" if world == 1 else "BASELINE configs[3] at 8 GPUs",
                    ("resnet18", 256, 32): "BASELINE configs[1]"}.get((args.arch, n_mask, n_img), "custom")
        # which library was timed: path, hash of the file, its build stamp, and whether that stamp is the hash of THIS tree's sources and
        # flags (__graft_entry__._source_hash).  A probe build (MPX_LIB_PATH / tools/with_lib.py; possibly timing-only) never carries a
        # BASELINE workload name
        bound = _lib.bound_library()
        bound["lib_stamp_matches_tree"] = bound["lib_stamp"] == g._source_hash(g.lib_sources(), g.HIPCC_FLAGS)
        if not bound["product_library"]:
            cfg_name = "custom (probe library)"
        conv_ms, conv_n = prof["ms"].get("conv", 0.0), prof["launches"].get("conv", 0)
        flops_per_batch = eng.flops_per_forward * batch
        roofline = None
        traffic_per_batch, traffic_source = pmc_traffic(args.arch, batch) if args.full else (None, None)
        if conv_n:
            # dominant kernel = conv_f16x3_kernel (all conv/fc launches).  achieved = algorithmic FLOPs
            # of the launches / their summed HIP-event durations; MFMA-issued FLOPs are 3x algorithmic.
            achieved = flops_per_batch * batches_profiled / (conv_ms * 1e-3) / 1e12
            roofline = {"bound": "mfma", "achieved": achieved, "peak": PEAK_F16_MFMA_TFLOPS, "unit": "TFLOP/s",
                        "frac": achieved / PEAK_F16_MFMA_TFLOPS,
                        # HBM bytes per conv launch = PMC bytes of the conv kernels per forward batch / conv launches per batch (a
                        # launch = one layer; 26 of them split their last round off into a second, small kernel dispatch)
                        "traffic": (traffic_per_batch / (conv_n / forwards_profiled)) if traffic_per_batch else None,
                        # NOT measured in this run: PMC counters need rocprofv3; the file holds the per-batch bytes of the same forward
                        "traffic_source": traffic_source, "traffic_bytes_per_forward_batch": traffic_per_batch,
                        "kernel": "conv_f16x3_kernel + conv3x3p_f16x3_kernel + conv3x3pp_f16x3_kernel + conv256_f16x3_kernel + conv256p_f16x3_kernel + convx_f16x3_kernel + convw_f16x3_kernel + btail_f16x3_kernel"
                                  + (" + stem_apply_kernel (conv1 + bn1 + relu + maxpool of all masks of an image from its superposition table)" if eng.stem == "table" else "")
                                  + " (all conv launches)", "launches": conv_n,
                        "avg_launch_us": conv_ms * 1e3 / conv_n,
                        # f16x3 issues three fp16 MFMA products per algorithmic product: at fp32-equivalent precision the
                        # path's own arithmetic ceiling is peak/3 (the north-star's 0.90 of 2.5 PF is out of reach by construction)
                        "f16x3_ceiling": F16X3_CEILING_TFLOPS, "frac_of_f16x3_ceiling": achieved / F16X3_CEILING_TFLOPS,
                        "mfma_issued_frac": 3 * achieved / PEAK_F16_MFMA_TFLOPS,
                        # the same algorithmic rate against the exact-fp32 MFMA peak: what an fp32-in / fp32-accumulate conv stack (the
                        # reference's arithmetic type) could reach at most on this chip
                        "f32_mfma_peak": PEAK_F32_MFMA_TFLOPS, "achieved_over_f32_mfma_peak": achieved / PEAK_F32_MFMA_TFLOPS,
                        # disclosure: with the stem by superposition conv1's 236 MFLOP per forward (1.5 % of the numerator) are delivered by an
                        # fp32 gather over per-image terms, not executed on the MFMA pipe; they stay in the ALGORITHMIC numerator
                        "stem": ("table: conv1 + bn1 + relu + maxpool of all masks of an image by superposition (mpx_stem_table_*); its launch is "
                                 "among the conv launches, its 1.5 % of the algorithmic FLOPs stay in the numerator") if eng.stem == "table" else "conv: K0 + MFMA stem + max pool",
                        "measured": "HIP events around every launch of one extra step after the timed region (%.2f forward batches of %d)" % (batches_profiled, batch),
                        "conv_ms_per_batch": conv_ms / max(batches_profiled, 1),
                        "timed_region_gpu_ms_per_batch": gpu_ms_timed / (args.steps * batches_per_step),
                        "other_kernels_ms_per_batch": {k: v / max(batches_profiled, 1) for k, v in prof["ms"].items() if k != "conv"}}
        line = {
            "metric": "masked-forward-passes/sec (224x224, %s)" % args.arch,
            "value": value, "unit": "masked-forward-passes/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None,
            "dtype": "f16x3 (split-fp16 MFMA, fp32 accumulate)" + ("; stem conv in fp32 by superposition over superpixels" if eng.stem == "table" else ""),
            "data": "synthetic (random-init torchvision-shaped weights, uniform-random u8 images, 14x14-block label map)",
            "config": {"workload": "%s, %d masks/image x %d images per GPU (%s; x%d GPUs)" % (args.arch, n_mask, n_img, cfg_name, world),
                       "images_per_gpu": n_img, "masks_per_image": n_mask, "forward_batch": batch, "num_cus": eng.num_cus,
                       "entry": "MaskedForwardEngine.score_packed", "stem": eng.stem,
                       "lib_path": os.path.relpath(bound["lib_path"], ROOT) if bound["product_library"] else bound["lib_path"],
                       "lib_sha256": bound["lib_sha256"], "lib_stamp": bound["lib_stamp"],
                       "lib_stamp_matches_tree": bound["lib_stamp_matches_tree"], "product_library": bound["product_library"],
                       "parallelism": "mask-batch shard x%d + one all_gather of scores" % world},
            "tflops_algorithmic": value * eng.flops_per_forward / 1e12,
            "full": args.full,
            "roofline": roofline,
        }
        # --full: CPU baseline on rank 0 at N=1 only (bounded sample) -- and the metric's second half on the same masks: the engine's
        # scores against the reference-style CPU loop
        base, parity = cpu_baseline(args.arch, args.cpu_masks, eng) if (args.full and world == 1 and args.cpu_masks > 0) else (None, None)
        line["cpu_baseline"] = base
        line["score_max_abs_delta"] = parity["score_max_abs_delta"] if parity else None
        line["argmax_agree"] = parity["argmax_agree"] if parity else None
        line["parity"] = parity
        print(json.dumps(line))
    eng.close()
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
