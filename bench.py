#!/usr/bin/env python
"""Headline benchmark: frames/s of the WVN hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W
        N > 1: either launched by torch.distributed.run (RANK / WORLD_SIZE in the environment), or -- when called plainly --
        bench.py re-executes itself under torch.distributed.run with N ranks on this node (it fails loudly if the node has
        fewer than N GPUs: it never prints an n_gpus it did not run on).

One "step" = one pass of the hot path over one batch of synthetic frames PER GPU (weak scaling; --scaling strong splits
the 64-frame batch over the ranks):
  --mode full (default; BASELINE.json configs[2]): 64 frames 448x448 -> ImageNet-normalise + patchify -> DINO ViT-S/8 (12 blocks),
      the frame AND its mirror image (the flip pass of the upstream Stego.get_code) -> STEGO head (90-d code, the two passes
      averaged) -> per-image cosine k-means (20 clusters) over the 448 x 448 bilinearly up-sampled code pixels -> segment maps ->
      per-segment mean pooling -> ONE optimisation step of the traversability MLP (forward, loss, backward, Adam) on the batch's
      segment rows, with the statistic / gradient all-reduces over RCCL when N > 1.  (--stego-reading patch: the opt-in fast form,
      one pass, k-means over the patch codes.)
  --mode backbone (configs[1]): --batch 32 frames through the ViT only (feature extraction).
  --mode dinov2   (configs[4]): DINOv2 ViT-B/14 at 518x518 (1370 tokens, LayerScale) + STEGO head, --batch 16 frames per GPU
                  (128 over 8 GPUs); meant for --precision fp8 (block linears on e4m3 MFMA), also runs in bf16 / exact.
  --precision mixed: the <= 1e-3 mode and the DEFAULT of --mode full (north_star: outputs within 1e-3 of the fp32 reference): every block linear
                     as fp16 hi * hi + two scaled e5m2 correction products (MX form, round 6; WVN_NO_MX=1: hi + lo split bf16 operands, three
                     MFMAs per product), the attention products on the fp16-operand kernel with q as two planes in the first six blocks -- the
                     cheapest mix the per-family error budget allows
  --precision exact: every product split (fp32-class results on the matrix pipe); --precision fp32: the FMA cross-check
  --precision fp16 : ONE fp16 value per MFMA operand (11 significand bits), fp32 accumulate / residual / statistics: the opt-in speed
                     path (tokens 4.5e-3 from the oracle)
  --precision bf16 : the same kernels with bf16 operands (8 significand bits; same speed, 8x the operand rounding)
Inputs (a pool of distinct batches) are resident in HBM before the timed region; weights are seeded synthetic (no network).
Prints ONE JSON line on rank 0 with `roofline` (dominant kernel = fused attention, HIP-event timed on the launch stream inside
the timed region).  A plain run does nothing else: it sets up, warms up, times the steps, writes --dump-outputs and prints the line.
--full adds `cpu_baseline` (the CPU oracle on a bounded sample of the same workload, rank 0, N = 1 only) and `parity`
(the GPU path against that oracle on the same frames: what BASELINE.md 4.5 asks to be reported with every speed number);
with --full the default run (N = 1, --mode full) also times more legs after the headline leg, each >= 20 steps, and reports them inside
the same line, each with its own roofline and parity:
  `fp16_speed`     : the SAME workload with --precision fp16 (the speed path; outside the 1e-3 clause, hence a leg and not `value`)
  `stego_fast`     : the opt-in fast form of the STEGO stage (one backbone pass, k-means over the patch codes, fused pooling), fp16 --
                     less work per frame by definition, reported as an option
  `backbone_b32`   : BASELINE configs[1] (ViT-S/8 448^2, batch 32, feature extraction only, fp16 operands)
  `dinov2_fp8`     : BASELINE configs[4], one GPU's share (DINOv2 ViT-B/14 518^2 + STEGO head, batch 16, fp8 block linears)
  `grid_mixed`     : SURVEY 8(d) C3-(i): the same 64 frames with `grid` segmentation (32-pixel cells, 196 segments per frame, ONE backbone pass,
                     12 544 MLP rows per step: the general learner path) in --precision mixed -- NOT the metric (north_star names the STEGO segmentation)
(--full --no-extra-legs skips them; A/B runs and N > 1 runs never run them).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_BF16_TFLOPS = 2500.0  # dense bf16 / fp16 MFMA peak, MI355X_MICROARCH.md
PEAK_FP8_TFLOPS = 5000.0   # dense fp8 MFMA peak (scaled K = 64 / 128 forms)
TRAFFIC_FILE = os.path.join(ROOT, "profiles", "attention_traffic.json")  # PMC-derived HBM bytes of the dominant kernel


def attention_traffic_per_launch(frames_per_launch, precision):
    """HBM bytes per attention launch from the committed rocprofv3 PMC passes (FETCH_SIZE x2 gfx950 correction + WRITE_SIZE,
    separate passes; the json says how it was collected).  Traffic of this kernel is proportional to the (frame, head) pairs
    of a launch, so the profiled figure is rescaled to this run's launch size.  None when no profile is committed."""
    try:
        t = json.load(open(TRAFFIC_FILE))
        if precision not in ("bf16", "fp16", "fp8"):   # fp16: the same kernel and byte counts as bf16 (16-bit operands)
            t = t[precision]   # sub-entry of the exact-mode kernel; the top level is the 16-bit-operand kernel
        return (t["fetch_bytes_corrected"] + t["write_bytes"]) * frames_per_launch / t["frames_per_launch"]
    except Exception:
        return None


def vit_flops_per_frame(S=448, P=8, D=384, depth=12):
    G = S // P
    N = G * G + 1
    per_block = 24 * N * D * D + 4 * N * N * D
    return depth * per_block + 2 * G * G * 3 * P * P * D, 4 * N * N * D  # (total, attention per block)


def linear_flops_per_frame(S=448, P=8, D=384, depth=12):
    """Algorithmic FLOPs of the four block linears (QKV, projection, fc1, fc2) of one frame pass: depth * 24 N D^2."""
    N = (S // P) ** 2 + 1
    return depth * 24 * N * D * D


# matrix-pipe work the block linears ISSUE per algorithmic product, in units of one fp16 / bf16 MFMA pass over it
LINEAR_ISSUE = {"fp16": 1.0, "bf16": 1.0, "exact": 3.0, "mixed": 2.0, "mixed_x3": 3.0, "fp8": 0.5, "fp32": None}


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50, help="timed steps of the headline leg (>= 1)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--mode", default="full", choices=["full", "backbone", "dinov2"])
    ap.add_argument("--batch", type=int, default=None, help="frames per GPU per step (full: 64, backbone: 32 = BASELINE configs[2] / [1])")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"],
                    help="weak: --batch frames per GPU; strong: --batch frames in all, split over the ranks")
    ap.add_argument("--size", type=int, default=448)
    ap.add_argument("--chunk", type=int, default=64, help="frames pushed through the backbone per launch sequence")
    ap.add_argument("--segmentation", default="stego", choices=["stego", "grid"])
    ap.add_argument("--stego-reading", default="upstream", choices=["upstream", "patch"],
                    help="'upstream' (default = the defaults of StegoInterface): the code averaged with the mirrored frame's (flip TTA, "
                         "two backbone passes per frame) and k-means over the H x H up-sampled code pixels, as the absent STEGO package "
                         "does it as published (parity unpinned); 'patch' = the opt-in fast form: single pass, k-means over the patch "
                         "codes (--full times it as the extra leg stego_fast)")
    ap.add_argument("--pool", type=int, default=4, help="distinct input batches cycled through the steps")
    ap.add_argument("--full", action="store_true",
                    help="after the headline leg: the CPU-oracle sample and parity blocks and, on the plain default workload, the extra legs "
                         "(a plain run measures the headline figure only)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU-oracle sample and the parity blocks")
    ap.add_argument("--attn-variant", type=int, default=None, help="A/B: 0 exact per-tile row max, 1 lazy (alarm on the row sums)")
    ap.add_argument("--no-fuse-proj", action="store_true", help="A/B: the attention projection as its own kernel instead of the fused MLP kernel's prologue")
    ap.add_argument("--no-fuse-qkv", action="store_true", help="A/B: LayerNorm kernel + QKV GEMM instead of the fused kernel")
    ap.add_argument("--no-fuse-mlp", action="store_true", help="A/B: run the block MLP as the un-fused fc1 / fc2 kernel pair")
    ap.add_argument("--cpu-frames", type=int, default=8, help="frames of the bounded CPU-oracle sample (about 15 s of CPU work)")
    ap.add_argument("--cpu-threads", type=int, default=32)
    ap.add_argument("--precision", default=None, choices=["fp16", "bf16", "mixed", "exact", "fp32", "fp8"],
                    help="default: mixed for --mode full (the <= 1e-3 headline), fp16 for --mode backbone / fast, fp8 for --mode dinov2")
    ap.add_argument("--no-extra-legs", action="store_true",
                    help="--full without the extra legs (no fp16_speed / stego_fast / grid_mixed / backbone_b32 / dinov2_fp8 legs)")
    ap.add_argument("--extra-steps", type=int, default=20, help="--full: timed steps of each extra leg (after 5 warm-up steps)")
    ap.add_argument("--backend", default=None, choices=["nccl", "gloo"],
                    help="process-group backend for N > 1 (default nccl = RCCL; gloo: the multi-process path on a box with one GPU, "
                         "all ranks on cuda:0 -- tests/test_gpu_distributed.py)")
    ap.add_argument("--force-collectives", action="store_true",
                    help="N = 1 only: a one-rank process group whose two all-reduces per step are issued for real (backend nccl: RCCL's "
                         "kernels on this GPU next to the persistent backbone kernels) -- `allreduce_ms` then says what a collective "
                         "waits and costs under the two-stream schedule (VERDICT r4 item 6)")
    ap.add_argument("--no-overlap", action="store_true",
                    help="run every step on one stream (default: the backbone of step i+1 runs on a second HIP stream while "
                         "clustering / pooling / the MLP step of step i -- small kernels that do not fill the GPU -- finish)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the headline leg's last timed step returned to its caller as DIR/<name>.npy "
                         "(float32; at most 64 MB in all: a fixed, seeded sample of each array when larger; the result line's 'dumped_outputs' "
                         "records every array's shape and whether it was sampled)")
    args = ap.parse_args(argv)
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("--steps must be >= 1 and --warmup >= 0")
    if args.batch is None:
        args.batch = {"full": 64, "backbone": 32, "dinov2": 16}[args.mode]
    if args.precision is None:
        # configs[2] (mode full): the <= 1e-3 mode -- north_star asks for outputs within 1e-3 of the fp32 reference, so THAT mode is
        # the headline and the fp16-operand speed path is an extra leg; configs[1] is quoted in bf16 (fp16
        # operands: >= that), configs[4] in fp8
        args.precision = {"dinov2": "fp8", "backbone": "fp16", "full": "mixed"}[args.mode]
    if args.mode == "dinov2":
        args.size, args.chunk = 518, min(args.chunk, args.batch)
    if args.precision == "fp8" and args.mode == "full":
        raise SystemExit("--precision fp8 is the configs[4] mode (--mode dinov2 / backbone); configs[2] is quoted in bf16")
    return args


def maybe_spawn(args):
    """`python bench.py --gpus N` without a torchrun environment: become the launcher."""
    if args.gpus <= 1 or "RANK" in os.environ:
        return
    import torch

    n = torch.cuda.device_count()
    if n < args.gpus and args.backend != "gloo":
        raise SystemExit(f"bench.py: --gpus {args.gpus} requested but this node exposes {n} GPU(s); refusing to print a line "
                         "for a configuration that did not run")
    port = 29500 + (os.getpid() % 2000)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    raise SystemExit(subprocess.call(cmd, env=env))


def make_pipeline(args, dev, precision=None, stego_reading=None):
    precision = precision or args.precision
    stego_reading = stego_reading or args.stego_reading
    from wild_visual_navigation_amd.feature_extractor import FeatureExtractor
    from wild_visual_navigation_amd.model import SimpleMLP
    from wild_visual_navigation_amd.traversability_estimator import MlpTrainer

    import torch

    if args.mode == "dinov2":
        from wild_visual_navigation_amd.backbone import synthetic_vit_state_dict
        from wild_visual_navigation_amd.feature_extractor.stego_interface import synthetic_stego_head

        fe = FeatureExtractor(dev, segmentation_type="stego", feature_type="stego", input_size=518, n_image_clusters=20,
                              precision=precision, max_chunk=args.chunk, backbone_type="vit_base", patch_size=14,
                              pretrained_weights=synthetic_vit_state_dict("vit_base", 14, pretrain_grid=37, seed=0, dinov2=True),
                              head_weights=synthetic_stego_head(768), allow_synthetic=True,
                              flip_tta=False)   # configs[4] names the backbone + STEGO head: ONE pass per frame (the class default would add the mirror pass)
    else:
        ftype = "stego" if (args.segmentation == "stego" and args.mode == "full") else "dino"
        seg = args.segmentation if args.mode == "full" else "grid"
        fe = FeatureExtractor(dev, segmentation_type=seg, feature_type=ftype, input_size=args.size,
                              backbone_type="vit_small", patch_size=8, n_image_clusters=20, precision=precision,
                              max_chunk=args.chunk, allow_synthetic=True, fuse_mlp=False if args.no_fuse_mlp else None,
                              fuse_qkv=False if args.no_fuse_qkv else None, fuse_proj=not args.no_fuse_proj,
                              flip_tta=stego_reading == "upstream",
                              cluster_resolution="pixel" if stego_reading == "upstream" else "patch")
    if args.attn_variant is not None:
        from wild_visual_navigation_amd import _lib
        _lib.lib().wvn_debug_attention_variant(args.attn_variant)
    if os.environ.get("WVN_QSPLIT_FORM"):   # A/B of the two-plane q's second plane: 2 = one scaled e5m2 MFMA per sub-tile (default), 1 = fp16 MFMAs (round 4)
        from wild_visual_navigation_amd import _lib
        _lib.lib().wvn_debug_attention_variant(16 + int(os.environ["WVN_QSPLIT_FORM"]))
    if os.environ.get("WVN_N384_PAIR"):   # A/B of the two forms of the fragment-major row-panel kernel (1 wave pair = default, 0 one wave per SIMD)
        from wild_visual_navigation_amd import _lib
        _lib.lib().wvn_debug_n384_pair(int(os.environ["WVN_N384_PAIR"]))
    if os.environ.get("WVN_KMEANS_ASSIGN_FORM"):   # A/B of the pixel k-means assignment kernels (5 packed VALU = default, 0 plain VALU, 1 screened MFMA)
        from wild_visual_navigation_amd import _lib
        _lib.lib().wvn_debug_kmeans_assign_form(int(os.environ["WVN_KMEANS_ASSIGN_FORM"]))
    torch.manual_seed(42)
    model = SimpleMLP(fe.feature_dim, [256, 32, 1], True).to(dev)
    return fe, model, MlpTrainer(model)


def hot_path_step(fe, trainer, img, labels_u, args, backbone_out=None, sink=None):
    """One pass: frames -> features/segments -> pooled rows -> one MLP optimisation step.  ``sink`` (a dict, or None): receives
    the device tensors the step hands its caller (no copy, no synchronisation)."""
    import torch

    from wild_visual_navigation_amd import ops

    feat, seg, nseg = fe.extract_batch(img, backbone_out=backbone_out)
    B, S, D = feat.shape
    rows_dev = None
    if args.segmentation == "stego":   # ids a frame's k-means did not produce are dropped -- on the device: the rows that exist
        x, u, rows_dev = ops.compact_segment_rows(feat, nseg, labels_u)   # move to the front, the count never visits the host
    else:
        x = feat.reshape(B * S, D)
        u = labels_u.reshape(B * S, 2)
    y_valid = u[:, 0] < 0.16  # 16 % labelled segments, like assets/graph/graph.pt (16 / 100)
    y = y_valid.float() * (0.5 + 0.5 * u[:, 1])
    losses = trainer.train_step(x, y, y_valid, rows_dev=rows_dev)
    if sink is not None:
        sink.update(features=feat, segments=seg, n_segments=nseg, losses=losses,
                    mlp_rows=rows_dev if rows_dev is not None else torch.tensor([x.shape[0]]))
    return losses, (rows_dev if rows_dev is not None else x.shape[0])


CU_SPLIT_DEFAULT = "none"   # "<a_hi>,<b_lo>[,rr|lin]" or "none": see TwoStreamPipeline


class TwoStreamPipeline:
    """Steps are independent through the backbone, so a throughput pipeline skews them by one: stream A runs the backbone
    (+ STEGO head) of step i+1 while stream B runs clustering, pooling and the MLP optimisation step (and, multi-GPU, its two
    all-reduces) of step i.  Every step still trains on its own frames' features; only the schedule changes.  A runs at most
    one step ahead of B."""

    def __init__(self, fe, trainer, args, dev, streams=None):
        import torch

        self.torch = torch
        self.fe, self.trainer, self.args = fe, trainer, args
        # stream B (the many small kernels of clustering / pooling / the learner) is served first: its workgroups then slot in as the
        # persistent backbone kernels of stream A release CUs, instead of queueing behind whole launches (measured in one call: equal
        # priorities 987 - 1004 frames/s, backbone first 1017, tail first 1039).  WVN_BENCH_STREAM_PRIO = ab | a | b for A/B runs.
        pa, pb = {"ab": (0, 0), "a": (-1, 0), "b": (0, -1)}[os.environ.get("WVN_BENCH_STREAM_PRIO", "b")]
        split = streams if streams is not None else os.environ.get("WVN_BENCH_CU_SPLIT", CU_SPLIT_DEFAULT)
        self.masked = []
        if split and split != "none":
            # PARTITION the chip instead: "<a_hi>,<b_lo>[,layout]" -- stream A (backbone) on CUs [0, a_hi) of every
            # XCD, stream B (clustering / pooling / learner) on CUs [b_lo, 32); scripts/ab_cu_mask.py measured the table in
            # profiles/r04*_ab_cu_mask.txt
            from wild_visual_navigation_amd import ops
            parts = split.split(",")
            a_hi, b_lo, layout = int(parts[0]), int(parts[1]), (parts[2] if len(parts) > 2 else "rr")
            ma = ops.MaskedStream(ops.cu_mask_words(0, a_hi, layout), dev) if a_hi < 32 else None
            mb = ops.MaskedStream(ops.cu_mask_words(b_lo, 32, layout), dev) if b_lo > 0 else None
            self.masked = [m for m in (ma, mb) if m is not None]
            self.a = ma.stream if ma else torch.cuda.Stream(device=dev, priority=pa)
            self.b = mb.stream if mb else torch.cuda.Stream(device=dev, priority=pb)
        else:
            self.a, self.b = torch.cuda.Stream(device=dev, priority=pa), torch.cuda.Stream(device=dev, priority=pb)
        self.pending = None     # (tokens, event) of a backbone stage already enqueued for the next step
        self.tail_done = None   # event: the previous step's tail has finished
        self.marks = []         # per-step end events (timing on), recorded on stream B

    def _enqueue_backbone(self, img):
        torch = self.torch
        if self.tail_done is not None:
            self.a.wait_event(self.tail_done)              # A runs at most one step ahead of B (bounded memory)
        with torch.cuda.stream(self.a):
            tok = self.fe.backbone_stage(img)
            tok.record_stream(self.b)
            ready = torch.cuda.Event()
            ready.record(self.a)
        return tok, ready

    def step(self, img, labels_u, next_img=None, sink=None):
        """Runs one step on ``img``; ``next_img`` (the following step's frames, None for the last step) gets its backbone
        stage enqueued FIRST (the tail itself no longer synchronises with the host: rows are compacted on the device)."""
        torch = self.torch
        tok, ready = self.pending if self.pending is not None else self._enqueue_backbone(img)
        self.pending = self._enqueue_backbone(next_img) if next_img is not None else None
        with torch.cuda.stream(self.b):
            self.b.wait_event(ready)
            out = hot_path_step(self.fe, self.trainer, img, labels_u, self.args, backbone_out=tok, sink=sink)
            self.tail_done = torch.cuda.Event(enable_timing=True)
            self.tail_done.record(self.b)
            self.marks.append(self.tail_done)
        return out

    def drain(self):
        cur = self.torch.cuda.current_stream()
        cur.wait_stream(self.a)
        cur.wait_stream(self.b)


def cpu_oracle_sample(args, fe):
    """CPU oracle (a PORT: PyTorch/numpy restatement of the reference algorithm, oracle/) on a bounded sample of the same
    workload -- `cpu_frames` frames through backbone + STEGO head + k-means + pooling, then one MLP step on their rows --
    timed on this box's host cores.  Returns (cpu_baseline dict, the oracle's intermediate results for the parity legs)."""
    import torch

    from oracle import interfaces as OI, kmeans_linear as OKL, mlp as OM, segments as OS, vit as OV

    n = args.cpu_frames
    # PyTorch's intra-op pool does not scale to the GPU box's 256 hardware threads for these matrix
    # sizes (256 threads ran ~20x slower than the 8-core survey probe); the thread count used is reported.
    torch.set_num_threads(min(os.cpu_count() or 1, args.cpu_threads))
    stego = fe.feature_type == "stego"
    bb = fe._extractor._bb if stego else fe._extractor._model
    P, heads = bb.patch, bb.heads
    sd = {k: v.detach().float().cpu() for k, v in bb._sd.items()}           # the weights the GPU model was built from
    head = {k: v.detach().float().cpu() for k, v in fe._extractor._head_sd.items()} if stego else None
    img = torch.rand(n, 3, args.size, args.size, generator=torch.Generator().manual_seed(1))
    G = args.size // P
    upstream = stego and args.mode == "full" and args.stego_reading == "upstream"
    t0 = time.perf_counter()
    rows, toks, codes, segs = [], [], [], []
    with torch.no_grad():
        for b in range(n):
            tok = OV.vit_tokens(sd, OI.normalize(img[b:b + 1]), P, heads)[:, 1:]
            toks.append(tok)
            if args.mode == "backbone":
                continue
            if stego:
                if upstream:   # the mirror pass of Stego.get_code: a second backbone pass
                    tok_m = OV.vit_tokens(sd, OI.normalize(img[b:b + 1]).flip(-1), P, heads)[:, 1:]
                    code = OI.stego_code_flip_average(head, tok, tok_m, G)
                else:
                    code = OI.stego_code_tokens(head, tok)
                codes.append(code)
                if args.mode == "dinov2":
                    continue
                if upstream:
                    lab = OI.relabel_ascending(OKL.kmeans_cosine_labels_pixels_linear(code[0].numpy(), G, args.size, 20))
                    seg = torch.from_numpy(lab).reshape(args.size, args.size).long()
                else:
                    lab = OI.relabel_ascending(OI.kmeans_cosine_labels(code[0].numpy(), 20))
                    seg = OI.upsample_nearest(torch.from_numpy(lab).reshape(1, G, G).int(), args.size)[0, 0].long()
                fmap = code.reshape(1, G, G, -1).permute(0, 3, 1, 2)
            else:
                seg = OS.segment_grid(args.size, args.size, 32)[0, 0]
                fmap = tok.reshape(1, G, G, -1).permute(0, 3, 1, 2)
            segs.append(seg)
            dense = OI.upsample_bilinear_ac(fmap, args.size)
            rows.append(OS.sparsify_features(dense, seg))
        if args.mode == "full":
            x = torch.cat(rows)
            gsel = torch.Generator().manual_seed(2)
            yv = torch.rand(x.shape[0], generator=gsel) < 0.16
            yv[0] = yv[1] = True
            y = yv.float() * (0.5 + 0.5 * torch.rand(x.shape[0], generator=gsel))
            st = OM.TrainState(OM.make_mlp_state_dict(x.shape[1]))
            OM.train_step(st, x, y, yv)
    dt = time.perf_counter() - t0
    segwhat = ("STEGO head with flip TTA (two backbone passes) + k-means over the code pixels" if upstream else
               "STEGO head + k-means over the patch codes" if stego else "grid segmentation")
    what = {"full": f"ViT-S/8 12 blocks fp32 + {segwhat} + pooling + 1 MLP step",
            "backbone": "ViT-S/8 12 blocks fp32", "dinov2": "DINOv2 ViT-B/14 12 blocks fp32 + STEGO head"}[args.mode]
    base = {"value": round(n / dt, 4), "unit": "frames/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": (f"{n} frames {args.size}x{args.size} through the CPU oracle ({what}), {dt:.1f} s wall; ViT / head / pooling / MLP = PyTorch fp32 "
                       f"on {torch.get_num_threads()} threads, k-means = the C restatement (fmaf chains in the definition's order, OpenMP) when "
                       "oracle/_build holds it, else numpy with a software fp32 fma (about 20 s per 448^2 frame instead of 0.1 s)")}
    orc = {"img": img, "toks": toks, "sd": sd, "head": head, "G": G, "P": P, "heads": heads,
           "codes": {args.stego_reading: codes}, "segs": {args.stego_reading: segs}}
    if upstream:   # (outside the timed sample) the same frames under the fast form, for the parity of the stego_fast leg
        with torch.no_grad():
            c2 = [OI.stego_code_tokens(head, t) for t in toks]
            s2 = [OI.upsample_nearest(torch.from_numpy(OI.relabel_ascending(OI.kmeans_cosine_labels(c[0].numpy(), 20))).reshape(1, G, G).int(),
                                      args.size)[0, 0].long() for c in c2]
        orc["codes"]["patch"], orc["segs"]["patch"] = c2, s2
    return base, orc


def gpu_parity(args, fe, dev, orc, precision, reading=None):
    """The GPU path in `precision` on the oracle's frames, with the SAME weights, compared stage by stage (the parity figures
    BASELINE.md 4.5 wants beside every speed number).  For k-means segment maps two figures: `seg_equal_frames` (end to end:
    the GPU's map against the oracle's map from the oracle's own code -- a 1e-4 difference in the code moves borderline
    points) and `seg_equal_given_gpu_code` (the integer stage alone: the oracle's k-means run on the GPU's code)."""
    import torch

    from oracle import interfaces as OI, kmeans_linear as OKL, segments as OS

    reading = reading or args.stego_reading
    n, G = args.cpu_frames, orc["G"]
    stego = fe.feature_type == "stego"
    bb = fe._extractor._bb if stego else fe._extractor._model
    with torch.no_grad():
        # the oracle's frames go through the GPU path inside a batch of the TIMED size (copies of themselves fill it): the library
        # picks its kernels by the number of rows, and the figures below are to describe the kernels the timed steps run
        reps = max(1, (args.batch or n) // n)
        gi = orc["img"].to(dev).repeat(reps, 1, 1, 1)
        gtok = bb.forward_tokens(gi)[:n].cpu()
        otok = torch.cat(orc["toks"])
        par = {"mode": precision, "frames": n, "against": ("oracle/ (CPU fp32 restatement; backbone / STEGO head parity unpinned; pixel k-means = the deterministic fixed-order definition of "
                           "oracle/kmeans_linear.py (the clustering through its linearity), which csrc/stego_linear.hip follows operation for operation)"),
               "gpu_batch": int(gi.shape[0]),
               "max_abs_tokens": float((gtok - otok).abs().max()), "rel_l2_tokens": float((gtok - otok).norm() / otok.norm())}
        ocodes = orc["codes"].get(reading) if stego else None
        if args.mode == "dinov2":
            gcode = fe.backbone_stage(gi)[:n].cpu()
            ocode = torch.cat(ocodes)
            par["max_abs_code"] = float((gcode - ocode).abs().max())
            par["rel_l2_code"] = float((gcode - ocode).norm() / ocode.norm())
        if args.mode == "full":
            feat, seg, nseg = fe.extract_batch(gi)
            feat, seg = feat[:n], seg[:n].cpu().long()
            oseg = torch.stack(orc["segs"][reading] if stego else orc["segs"][args.stego_reading])
            same = [bool(torch.equal(seg[b], oseg[b])) for b in range(n)]
            par["seg_equal_frames"] = f"{sum(same)}/{n}"
            par["seg_pixel_agreement"] = float((seg == oseg).float().mean())
            if stego:
                par["stego_reading"] = reading
                gcode = fe._extractor.feature_tokens[:n].cpu()
                par["max_abs_code"] = float((gcode - torch.cat(ocodes)).abs().max())
                # the integer stage on identical input: bit-exact by construction (tests pin it too).  The pixel-resolution oracle is
                # the C restatement (0.7 s per frame); without the built library (numpy: 25 s per frame) one frame is checked
                m = n if (reading == "patch" or OI._oracle_lib() is not None) else 1
                given = 0
                for b in range(m):
                    if reading == "upstream":
                        want = torch.from_numpy(OI.relabel_ascending(OKL.kmeans_cosine_labels_pixels_linear(gcode[b].numpy(), G, args.size, 20))
                                                ).reshape(args.size, args.size).long()
                    else:
                        lab = OI.relabel_ascending(OI.kmeans_cosine_labels(gcode[b].numpy(), 20))
                        want = OI.upsample_nearest(torch.from_numpy(lab).reshape(1, G, G).int(), args.size)[0, 0].long()
                    given += int(torch.equal(seg[b], want))
                par["seg_equal_given_gpu_code"] = f"{given}/{m}"
                if reading == "upstream" and OI._oracle_lib() is not None:
                    # the same check against the DIRECT statement (oracle/interfaces.py::kmeans_cosine_labels_pixels: every pixel's row re-created and
                    # multiplied out -- the reading of the reference's postprocess that has no tiling co-designed with the kernel), on the GPU's own code
                    nd = min(n, 2)
                    agree = []
                    for b in range(nd):
                        wd = torch.from_numpy(OI.relabel_ascending(OI.kmeans_cosine_labels_pixels(gcode[b].numpy(), G, args.size, 20))).reshape(args.size, args.size).long()
                        agree.append(float((seg[b] == wd).float().mean()))
                    par["seg_pixel_agreement_with_direct_form_given_gpu_code"] = {"frames": nd, "min": min(agree), "mean": sum(agree) / nd}
                if reading == "upstream" and OI._oracle_lib() is not None:
                    # what "bit-exact segment maps" means behind a float backbone (oracle/segmap_agreement.py): every pixel where the maps
                    # differ lies within the MEASURED float tolerance of an oracle decision boundary: margin <= 2 (eps_x + eps_c)
                    from oracle import segmap_agreement as SA
                    nf = min(n, 4)
                    rs = [SA.analyse(ocodes[b][0].numpy(), gcode[b].numpy(), G, args.size, 20) for b in range(nf)]
                    hist = [sum(r["margin_over_eps_hist"][i] for r in rs) for i in range(7)]
                    par["seg_tolerance"] = {
                        "frames": nf, "all_mismatches_within_float_tolerance": all(r["within_float_tolerance"] for r in rs),
                        "mismatching_pixels": sum(r["mismatching"] for r in rs), "max_margin": max(r["max_margin"] for r in rs),
                        "min_bound_2eps": min(r["bound_2eps"] for r in rs), "max_eps_x": max(r["eps_x"] for r in rs),
                        "max_eps_c": max(r["eps_c"] for r in rs),
                        "margin_over_eps_histogram": {"edges": [0, 0.01, 0.03, 0.1, 0.3, 1.0, 2.0, "inf"], "counts": hist}}
            # pooled features: the oracle's dense features pooled over the GPU's own segment map (so that the figure measures
            # the features, not a label permutation, when the maps differ)
            worst = 0.0
            for b in range(n):
                fmap = (ocodes[b] if stego else orc["toks"][b]).reshape(1, G, G, -1).permute(0, 3, 1, 2)
                want = OS.sparsify_features(OI.upsample_bilinear_ac(fmap, args.size), seg[b])
                got = feat[b, : want.shape[0]].cpu()
                ok = ~torch.isnan(want).any(1)
                worst = max(worst, float((got[ok] - want[ok]).abs().max()))
            par["max_abs_pooled"] = worst
    return par


def percentiles(xs):
    xs = sorted(xs)
    if not xs:
        return None
    pick = lambda q: xs[min(len(xs) - 1, max(0, int(round(q * (len(xs) - 1)))))]
    return {"median": round(statistics.median(xs), 3), "p10": round(pick(0.1), 3), "p90": round(pick(0.9), 3)}


PARITY_PRECISION = "mixed"   # the precision of the `parity_mode` leg: the cheapest mode that meets the 1e-3 token clause
KERNEL_NAME = {"fp16": "attention_bf16_kernel (fp16-operand build)", "bf16": "attention_bf16_kernel", "exact": "attention_x3_kernel",
               "mixed": "attention_bf16_kernel (fp16-operand build, hi + lo plane output)",
               "fp32": "attention_f32_kernel", "fp8": "attention_bf16_kernel"}
DTYPE = {"fp16": "f16", "bf16": "bf16", "exact": "bf16x3 (hi+lo split operands, fp32-class)", "fp32": "f32",
         "mixed": ("fp16 + e5m2-MX-correction linears (a w = a_h w_h + 2^-12 (a_h8 w_l8 + a_l8 w_h8); ~16 significand bits per product) + f16 attention products "
                   "(two-plane q in the first six blocks), fp32 accumulate / residual (<= 1e-3 parity mode)"),
         "fp8": "fp8-e4m3 linears (per-token / per-channel scales), bf16 attention, fp32 residual"}


def timed_leg(args, dev, world, rank, steps, warmup, precision, stego_reading, pool, labels, B, capture=False):
    """`warmup` untimed steps, then exactly `steps` steps between barrier + synchronize pairs.  Returns the leg's figures (the
    headline leg's go to the top level of the JSON line, the extra legs' into their own objects).  ``capture``: also return, as
    host numpy arrays under "outputs", what the LAST timed step handed its caller (plus the MLP parameters after it)."""
    import torch

    from wild_visual_navigation_amd import distributed as D, ops

    fe, model, trainer = make_pipeline(args, dev, precision, stego_reading)
    backbone_only = args.mode in ("backbone", "dinov2")
    bb = (fe._extractor._bb if fe.feature_type == "stego" else fe._extractor._model) if backbone_only else None
    pipe = None if (args.no_overlap or backbone_only) else TwoStreamPipeline(fe, trainer, args, dev)
    marks = []

    def run_step(i, last, sink=None):
        img, lab = pool[i % len(pool)], labels[i % len(pool)]
        if args.mode == "dinov2":
            out = (fe.backbone_stage(img), 0)          # ViT-B/14 + STEGO head -> 90-d code tokens
        elif backbone_only:
            out = (bb.forward_tokens(img), 0)
        elif pipe is None:
            out = hot_path_step(fe, trainer, img, lab, args, sink=sink)
        else:
            return pipe.step(img, lab, next_img=None if last else pool[(i + 1) % len(pool)], sink=sink)
        if sink is not None and backbone_only:
            sink["tokens"] = out[0]
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        marks.append(e)
        return out

    for i in range(warmup):
        run_step(i, i == warmup - 1)      # the pipeline is empty again when the timed region starts
    if pipe is not None:
        pipe.drain()
        pipe.marks.clear()
    marks.clear()
    torch.cuda.synchronize()
    D.barrier()
    ops.prof_enable(True)
    trainer.comm_events = [] if (world > 1 or D.is_parallel()) else None
    torch.cuda.synchronize()
    start = torch.cuda.Event(enable_timing=True)
    start.record()
    t0 = time.perf_counter()
    rows, losses = 0, None
    sink = {} if capture else None
    for i in range(steps):   # exactly `steps` backbone stages and `steps` tails in the timed region
        losses, rows = run_step(i, i == steps - 1, sink if i == steps - 1 else None)
    if pipe is not None:
        pipe.drain()
    torch.cuda.synchronize()
    D.barrier()
    dt = time.perf_counter() - t0
    ops.prof_enable(False)
    prof = ops.prof_collect()
    outputs = None
    if capture:   # copied before anything else runs on this pipeline (the oracle parity legs reuse its buffers)
        if not backbone_only:
            sink["mlp_params"] = model.flat_params()
        outputs = {k: v.detach().cpu().numpy() for k, v in sink.items()}
    dt = D.max_over_ranks(dt, dev)
    ends = pipe.marks if pipe is not None else marks
    step_ms, prev = [], start
    for e in ends:
        step_ms.append(prev.elapsed_time(e))
        prev = e
    comm_ms = None
    if trainer.comm_events:
        per = [a.elapsed_time(b) for a, b in trainer.comm_events]
        comm_ms = {"per_step_total": round(sum(per) / steps, 4), "stats_allreduce": percentiles(per[0::2]),
                   "grad_allreduce": percentiles(per[1::2])}
        comm_ms["per_step_total"] = D.max_over_ranks(comm_ms["per_step_total"], dev)
    if torch.is_tensor(rows):
        rows = int(rows.item())       # (after the timed region: the count lived on the device)
    # deterministic replicas (trainer.py): after the timed steps every rank must hold the same parameters, Adam moments and losses, bit
    # for bit -- checked with MIN / MAX all-reduces of their images
    replicas_ok = None
    if (world > 1 or D.is_parallel()) and not backbone_only:
        replicas_ok = D.replicas_identical(model.flat_params(), trainer.m, trainer.v, losses)
        assert replicas_ok, "the ranks' MLP replicas differ after the timed steps"
    loss_val = float(losses[0].item()) if not backbone_only else None

    total_frames = (args.batch if args.scaling == "strong" else world * B) * steps
    total_flops, attn_flops_block = (vit_flops_per_frame(518, 14, 768) if args.mode == "dinov2" else vit_flops_per_frame(args.size))
    passes = 2 if (stego_reading == "upstream" and args.mode == "full" and args.segmentation == "stego") else 1   # flip TTA
    att_ms, att_n = prof["attention"]
    frames_per_launch = (B * steps * 12 * passes) / max(att_n, 1)  # 12 attention launches per frame-chunk and pass
    att_avg_ms = att_ms / max(att_n, 1)
    att_tflops = attn_flops_block * frames_per_launch / (att_avg_ms * 1e-3) / 1e12 if att_n else 0.0
    roof = {"bound": "mfma", "kernel": KERNEL_NAME[precision], "achieved": round(att_tflops, 1), "peak": PEAK_BF16_TFLOPS,
            "unit": "TFLOP/s", "frac": round(att_tflops / PEAK_BF16_TFLOPS, 4),
            "traffic": attention_traffic_per_launch(frames_per_launch, precision), "avg_launch_ms": round(att_avg_ms, 4),
            "algorithmic_flops_per_launch": attn_flops_block * frames_per_launch}
    if precision == "mixed":  # the attention products run single fp16; the profiled traffic is the fp16 kernel's + the second output plane
        roof["traffic"] = attention_traffic_per_launch(frames_per_launch, "fp16")
        if roof["traffic"] is not None:
            roof["traffic"] += frames_per_launch * 3152 * 384 * 2
    if precision == "exact":  # three MFMAs per algorithmic product: what the matrix pipe actually issues
        roof["mfma_issued"] = round(3 * att_tflops, 1)
        roof["frac_issued"] = round(3 * att_tflops / PEAK_BF16_TFLOPS, 4)
    # the block linears as a family (QKV + projection + fc1 + fc2; HIP-event time of their spans inside the timed region): in the <= 1e-3 mode they are
    # the larger share of the step and sit far lower against the roof than the attention kernel -- VERDICT r5 item 4 asks to see both
    lin_ms = sum(prof[k][0] for k in ("qkv_gemm", "proj_gemm", "fc1_gemm", "fc2_gemm") if k in prof)
    lin_launches = sum(prof[k][1] for k in ("qkv_gemm", "proj_gemm", "fc1_gemm", "fc2_gemm") if k in prof)
    lin_flops = (linear_flops_per_frame(518, 14, 768) if args.mode == "dinov2" else linear_flops_per_frame(args.size)) * passes * B * steps
    mxkey = "mixed_x3" if (precision == "mixed" and os.environ.get("WVN_NO_MX")) else precision
    lin = None
    if lin_ms > 0:
        lin_tf = lin_flops / (lin_ms * 1e-3) / 1e12
        peak = PEAK_FP8_TFLOPS if precision == "fp8" else PEAK_BF16_TFLOPS
        lin = {"kernels": "QKV + projection + fc1 + fc2 of all blocks (" + {"mixed": "gemm_a384_mx2 (two workgroups per CU) / gemm_n384_mx_pair", "mixed_x3": "gemm_a384_x3 / gemm_n384_x3_frag_pair",
                                                                              "exact": "gemm_a384_x3 / gemm_n384_x3", "fp8": "gemm_a768_fp8 (QKV, projection, fc1: A-stationary) + gemm_fp8_dma (fc2: DMA-fed 128 x 128 tiles, MX block-scaled A) + row quantisers",
                                                                              "fp32": "gemm_f32"}.get(mxkey, "qkv_fused + mlp_fused") + ")",
               "ms_per_step": round(lin_ms / steps, 3), "launches_per_step": round(lin_launches / steps, 1), "achieved": round(lin_tf, 1), "peak": peak, "unit": "TFLOP/s",
               "frac": round(lin_tf / peak, 4), "algorithmic_flops_per_step": lin_flops / steps}
        iss = LINEAR_ISSUE.get(mxkey)
        if iss is not None and precision != "fp8":
            lin["issued_per_product"] = iss
            lin["frac_issued"] = round(iss * lin_tf / PEAK_BF16_TFLOPS, 4)
        roof["linears"] = lin
        roof["attention_ms_per_step"] = round(att_ms / steps, 3)
    if precision == "fp8" and lin is not None:
        # configs[4]: the leg's dominant family is the fp8 linears (6.5 of its 9.2 ms), priced against the 5 PF fp8 peak; the attention kernel's own figure stays beside it
        att = dict(roof)
        att.pop("linears", None)
        roof = {"bound": "mfma", "kernel": lin["kernels"], "achieved": lin["achieved"], "peak": PEAK_FP8_TFLOPS, "unit": "TFLOP/s", "frac": lin["frac"],
                "traffic": None, "ms_per_step": lin["ms_per_step"], "algorithmic_flops_per_step": lin["algorithmic_flops_per_step"], "attention": att}
    return {"fe": fe, "pipe": pipe, "rows": rows, "dt": dt, "value": round(total_frames / dt, 2),
            "ms_per_step": round(dt / steps * 1e3, 3), "step_ms": percentiles(step_ms),
            "backbone_tflops": round(total_flops * passes * total_frames / dt / 1e12 / world, 1), "final_loss": loss_val,
            "roofline": roof, "kernel_ms": {k: {"ms_total": round(v[0], 3), "launches": v[1]} for k, v in prof.items()},
            "allreduce_ms": comm_ms, "replicas_identical": replicas_ok, "steps": steps, "warmup": warmup, "outputs": outputs}


DUMP_BUDGET_BYTES = 64 << 20


def dump_outputs(path, outputs, budget=DUMP_BUDGET_BYTES):
    """Write ``outputs`` ({name: numpy array}) as path/<name>.npy in float32 (float64 arrays stay float64), ``budget`` bytes at
    most in all.  Arrays of up to 256 KB are written whole; when the rest do not fit, each of them is replaced by a sample, its
    share of the budget, at flat indices drawn with a fixed seed from the array's size (so two runs with the same arguments
    sample the same elements).  Returns {name: shape, dtype, sampled} for the result line."""
    import numpy as np

    os.makedirs(path, exist_ok=True)
    arrs = {k: np.ascontiguousarray(v, dtype=np.float64 if v.dtype == np.float64 else np.float32) for k, v in outputs.items()}
    small = 256 << 10
    room = budget - (64 << 10) - sum(a.nbytes for a in arrs.values() if a.nbytes <= small)   # 64 KB: the .npy headers
    large = sum(a.nbytes for a in arrs.values() if a.nbytes > small)
    manifest = {}
    for name, a in sorted(arrs.items()):
        entry = {"shape": list(a.shape), "dtype": str(a.dtype), "sampled": False}
        if a.nbytes > small and large > room:
            cap = (room * a.nbytes // large) // a.itemsize
            if a.size > cap:
                idx = np.sort(np.random.default_rng(0).choice(a.size, size=cap, replace=False))
                a = a.reshape(-1)[idx]
                entry.update(sampled=True, sample_size=int(cap), sample_seed=0)
        np.save(os.path.join(path, name + ".npy"), a)
        manifest[name] = entry
    return manifest


def full_extras(args, world):
    """What runs after the headline leg: (the extra legs, the CPU-oracle sample + parity blocks).  A plain run: neither.  The
    extra legs: --full on the plain default workload only (N = 1, configs[2], no A/B switch); the oracle: --full, N = 1."""
    legs = (args.full and world == 1 and args.mode == "full" and args.segmentation == "stego" and args.stego_reading == "upstream"
            and not args.no_extra_legs and args.attn_variant is None
            and not (args.no_fuse_proj or args.no_fuse_qkv or args.no_fuse_mlp or args.no_overlap))
    return legs, args.full and world == 1 and not args.no_cpu_baseline


def main():
    args = parse()
    maybe_spawn(args)
    import torch

    from wild_visual_navigation_amd import distributed as D

    rank, world, local = D.init_from_env(args.backend, force_collectives=args.force_collectives and args.gpus == 1)
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    assert torch.cuda.is_available(), "bench.py needs a GPU (the HIP path has no CPU fallback)"
    if args.backend == "gloo":
        local = local % max(torch.cuda.device_count(), 1)   # more ranks than GPUs (one-GPU box): ranks share devices
    dev = torch.device(f"cuda:{local}")
    torch.cuda.set_device(dev)
    ranks_seen = world
    if world > 1:   # prove the process group spans `world` ranks (over RCCL unless --backend gloo) before timing anything
        t = torch.ones(1, device=dev)
        torch.distributed.all_reduce(t)
        ranks_seen = int(t.item())
        assert ranks_seen == world, f"all-reduce saw {ranks_seen} ranks, expected {world}"
    if args.scaling == "strong":
        b0, b1 = D.shard_range(args.batch, rank, world)
        B = b1 - b0
        if B <= 0:
            raise SystemExit("--scaling strong: more ranks than frames")
    else:
        B = args.batch
    gen = torch.Generator().manual_seed(1000 + rank)
    pool = [torch.rand(B, 3, args.size, args.size, generator=gen).to(dev) for _ in range(max(1, args.pool))]  # resident in HBM
    n_lab = 20 if args.segmentation == "stego" else (args.size // 32) ** 2
    labels = [torch.rand(B, n_lab, 2, generator=gen).to(dev) for _ in range(len(pool))]
    backbone_only = args.mode in ("backbone", "dinov2")

    head = timed_leg(args, dev, world, rank, args.steps, args.warmup, args.precision, args.stego_reading, pool, labels, B,
                     capture=args.dump_outputs is not None)
    dumped = None
    if rank == 0 and args.dump_outputs is not None:
        dumped = dump_outputs(args.dump_outputs, head.pop("outputs"))
    # the extra legs (the batches unchanged) and the CPU oracle: --full only
    plain, oracle_sample = full_extras(args, world)
    legs = {}
    SPEED = "fp16"   # the opt-in speed path's operand format
    if plain and args.precision in ("exact", "mixed"):
        legs["fp16_speed"] = timed_leg(args, dev, world, rank, max(20, args.extra_steps), 5, SPEED, "upstream", pool, labels, B)
    if plain and args.precision not in ("exact", "mixed"):
        legs["parity_mode"] = timed_leg(args, dev, world, rank, max(20, args.extra_steps), 5, PARITY_PRECISION, "upstream", pool, labels, B)
    if plain:
        legs["stego_fast"] = timed_leg(args, dev, world, rank, max(20, args.extra_steps), 5, SPEED, "patch", pool, labels, B)
        # the other two single-GPU configurations of BASELINE.json, on the kernels as they are today: configs[1]
        # (backbone only, batch 32) and configs[4]'s per-GPU share (DINOv2 ViT-B/14 518^2 fp8 + STEGO head, 16 frames per GPU)
        # `grid` segmentation (cell 32: 196 segments per frame, one backbone pass, 12 544 MLP rows -- the general learner path) in the
        # <= 1e-3 mode; labelled as what it is: NOT the metric (north_star: STEGO seg)
        ag = argparse.Namespace(**vars(args)); ag.segmentation, ag.precision = "grid", "mixed"
        labels_g = [torch.rand(B, (args.size // 32) ** 2, 2, generator=gen).to(dev) for _ in range(len(pool))]
        legs["grid_mixed"] = timed_leg(ag, dev, world, rank, max(20, args.extra_steps), 5, "mixed", "upstream", pool, labels_g, B)
        legs["grid_mixed"]["args"] = ag
        a1 = argparse.Namespace(**vars(args)); a1.mode, a1.batch, a1.precision = "backbone", 32, "fp16"
        legs["backbone_b32"] = timed_leg(a1, dev, world, rank, 20, 5, "fp16", "upstream", [p[:32] for p in pool], labels, 32)
        legs["backbone_b32"]["args"] = a1
        a4 = argparse.Namespace(**vars(args)); a4.mode, a4.batch, a4.precision, a4.size, a4.chunk = "dinov2", 16, "fp8", 518, 16
        pool4 = [torch.rand(16, 3, 518, 518, generator=gen).to(dev) for _ in range(2)]
        legs["dinov2_fp8"] = timed_leg(a4, dev, world, rank, 20, 5, "fp8", "upstream", pool4, labels, 16)
        legs["dinov2_fp8"]["args"] = a4
        del pool4

    if rank == 0:
        rows, chunk = head["rows"], min(args.chunk, B)
        lowp16 = args.precision in ("bf16", "fp16")
        if args.mode == "dinov2":
            metric = "frames/sec (518x518 DINOv2 ViT-B/14 + STEGO head)"
            workload = (f"BASELINE configs[4]: DINOv2 ViT-B/14 518x518 batch={B}/GPU (1370 tokens, LayerScale) + STEGO head -> 90-d "
                        f"code; block linears in {args.precision}")
        elif backbone_only:
            metric = "frames/sec (448x448 DINO-ViT-S/8 feature extraction)"
            workload = f"BASELINE configs[1]: DINO ViT-S/8 {args.size}x{args.size} batch={B}/GPU, feature extraction only"
        else:
            metric = "frames/sec (448x448 DINO-ViT-S/8 + seg + MLP train-step)"
            segdesc = ("grid segmentation (32-pixel cells)" if args.segmentation != "stego" else
                       "STEGO head with flip TTA (two backbone passes per frame: the frame and its mirror) + per-image cosine k-means "
                       "over the 448x448 up-sampled code pixels (20 clusters; evaluated through its linearity: a similarity table per pass interpolated per pixel, "
                       "centroid sums from summed tap weights -- the dense code never exists) -- the defaults of "
                       "StegoInterface = the absent STEGO package's get_code / postprocess as published"
                       if args.stego_reading == "upstream" else
                       "STEGO head + per-image cosine k-means (20 clusters, at patch resolution, single pass: no flip TTA -- the opt-in "
                       "fast form of StegoInterface, NOT its defaults)")
            workload = (f"BASELINE configs[2]: DINO ViT-S/8 {args.size}x{args.size} batch={B}/GPU + {segdesc} + "
                        f"{'fused' if args.stego_reading == 'patch' or args.segmentation != 'stego' else 'general (bilinear-weight)'} segment "
                        f"pooling + 1 traversability-MLP Adam step on {rows} rows/GPU")
        out = {
            "metric": metric,
            "value": head["value"],
            "unit": "frames/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": head["ms_per_step"],
            "higher_is_better": True,
            "scaling": args.scaling,
            "vs_baseline": None,
            "dtype": DTYPE[args.precision],
            "data": "synthetic",
            "config": {"workload": workload, "frames_per_gpu_per_step": B, "backbone_chunk": chunk, "input_pool": len(pool),
                       "parallelism": f"dp{world} (frame sharding, {'gloo' if args.backend == 'gloo' else 'RCCL'} all-reduce of MLP statistics + gradients)",
                       "ranks_seen": ranks_seen,
                       "block_kernels": ("per block: LayerNorm-on-load QKV (A-stationary, MX) | attention (MX planes out) | projection (row panel, MX; leaves the LayerNorm statistics) | "
                                         "LayerNorm-on-load fc1 + GELU (MX planes out) | fc2 (row panel, MX; leaves the next block's statistics): five launches, no LayerNorm kernel"
                                         if (args.precision == "mixed" and args.mode == "full" and not os.environ.get("WVN_NO_MX")) else
                                         "separate LayerNorm / GEMM kernels" if not lowp16 or args.mode == "dinov2" else
                                         "LayerNorm+QKV: %s; proj+LayerNorm+MLP: %s (kernel_ms: a fused kernel is booked under its first stage, "
                                         "qkv_gemm / fc1_gemm)" % ("separate" if args.no_fuse_qkv else "one kernel",
                                                                     "separate" if args.no_fuse_mlp else
                                                                     ("MLP fused, projection separate" if args.no_fuse_proj else "one kernel"))),
                       "schedule": "one stream" if head["pipe"] is None else
                                   "two HIP streams: backbone of step i+1 overlaps clustering / pooling / MLP step of step i (the second stream at high priority)"},
            "step_ms": head["step_ms"],
            "backbone_tflops": head["backbone_tflops"],
            "final_loss": head["final_loss"],
            "roofline": head["roofline"],
            "kernel_ms": head["kernel_ms"],
            "precision_mode": args.precision,
        }
        if dumped is not None:
            out["dumped_outputs"] = {"dir": args.dump_outputs, "arrays": dumped}
        if head["allreduce_ms"] is not None:
            out["allreduce_ms"] = head["allreduce_ms"]
            if args.force_collectives and world == 1:
                out["collectives_forced"] = ("one-rank process group: both all-reduces of every step issued for real (RCCL kernels on this GPU, "
                                             "on the tail stream at high priority, next to the persistent backbone kernels)")
            out["replicas_identical_after_timed_steps"] = head["replicas_identical"]
        orc = None
        if oracle_sample:
            out["cpu_baseline"], orc = cpu_oracle_sample(args, head["fe"])
            out["parity"] = gpu_parity(args, head["fe"], dev, orc, args.precision)
        for name, leg in legs.items():
            o = {"value": leg["value"], "unit": "frames/s", "ms_per_step": leg["ms_per_step"], "steps": leg["steps"],
                 "warmup": leg["warmup"], "step_ms": leg["step_ms"], "backbone_tflops": leg["backbone_tflops"],
                 "roofline": leg["roofline"], "kernel_ms": leg["kernel_ms"]}
            if name == "grid_mixed":
                la = leg["args"]
                o["dtype"] = DTYPE["mixed"]
                o["workload"] = (f"SURVEY 8(d) C3-(i) -- NOT the metric (north_star names the STEGO segmentation): DINO ViT-S/8 448x448 batch={B} + grid segmentation (32-pixel cells: 196 "
                                 f"segments per frame, ONE backbone pass per frame) + fused segment pooling of the 384-d tokens + 1 traversability-MLP Adam step on {leg['rows']} rows "
                                 "(the general learner path: split-K GEMM phases, not the <= 2048-row fused step), --precision mixed")
                if not args.no_cpu_baseline:
                    la.cpu_frames = 2
                    _, orc_g = cpu_oracle_sample(la, leg["fe"])
                    o["parity"] = gpu_parity(la, leg["fe"], dev, orc_g, "mixed")
                out[name] = o
                continue
            if name in ("backbone_b32", "dinov2_fp8"):
                la = leg["args"]
                o["dtype"] = DTYPE[la.precision]
                o["workload"] = ("BASELINE configs[1]: DINO ViT-S/8 448x448 batch=32, feature extraction only (fp16 operands, fp32 accumulate)"
                                 if name == "backbone_b32" else
                                 "BASELINE configs[4], one GPU's share: DINOv2 ViT-B/14 518x518 batch=16 (1370 tokens, LayerScale) + STEGO head -> "
                                 "90-d code, one backbone pass per frame (no flip TTA); block linears in fp8-e4m3: QKV / projection / fc1 on the A-stationary K = 768 kernel, fc2 (K = 3072) on DMA-fed 128 x 128 tiles at three workgroups per CU with its A operand (the hidden activation) as e4m3 + MX block scales straight from fc1's epilogue")
                if not args.no_cpu_baseline:   # its own bounded oracle sample (2 frames): other weights / another architecture
                    la.cpu_frames = 2
                    _, orc_l = cpu_oracle_sample(la, leg["fe"])
                    o["parity"] = gpu_parity(la, leg["fe"], dev, orc_l, la.precision)
                out[name] = o
                continue
            if name == "fp16_speed":
                o["dtype"] = DTYPE[SPEED]
                o["workload"] = ("the headline workload on the opt-in SPEED path (--precision fp16: one fp16 value per MFMA operand, fp32 "
                                 "accumulate): tokens 4.5e-3 from the fp32 oracle -- outside the north star's 1e-3 clause, which is why it is a leg "
                                 "and not `value`")
                if orc is not None:
                    o["parity"] = gpu_parity(args, leg["fe"], dev, orc, SPEED, "upstream")
            elif name == "parity_mode":
                o["dtype"] = DTYPE[PARITY_PRECISION]
                o["workload"] = (f"the headline workload with --precision {PARITY_PRECISION}: the <= 1e-3 parity path (every block linear as fp16 hi * hi + two scaled "
                                 "e5m2 correction products; the attention products on the fp16 kernel: the mix the per-family error budgets of "
                                 "profiles/r04a_error_budget_*.md / r06_error_budget.md select)")
                if orc is not None:
                    o["parity"] = gpu_parity(args, leg["fe"], dev, orc, PARITY_PRECISION, "upstream")
            else:
                o["dtype"] = DTYPE[SPEED]
                o["workload"] = ("the opt-in fast form of the STEGO stage (StegoInterface(flip_tta=False, cluster_resolution='patch')): ONE "
                                 "backbone pass per frame, per-image cosine k-means over the 56x56 patch codes (labels nearest-upsampled: "
                                 f"patch-aligned segments), fused segment pooling, 1 MLP Adam step on {leg['rows']} rows -- less work than "
                                 "the headline by definition; reported as an option, not as the metric")
                if orc is not None:
                    o["parity"] = gpu_parity(args, leg["fe"], dev, orc, SPEED, "patch")
            out[name] = o
        # RCCL prints its version banner through C stdio (flushed at exit when stdout is a pipe): flush it now so that the JSON line
        # is the LAST line of this process's output
        sys.stdout.flush()
        try:
            import ctypes

            ctypes.CDLL(None).fflush(None)
        except Exception:  # noqa: BLE001
            pass
        print(json.dumps(out), flush=True)
    D.barrier()
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
