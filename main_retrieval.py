#!/usr/bin/env python
"""DDP entry point for the similarity / loss path (the reference's main.py:189-437, launched in its
README as main_retrieval.py).  Same flag names, same per-epoch sequence
  load memory bank -> train epoch -> eval -> save -> clear bank,
same training-step contract (trainer.py:66-203): model(...) -> 5 losses -> backward ->
clip_grad_norm_(1.0) -> optimizer step -> clamp logit_scale <= ln 100 -> reduce the 5 scalars to
rank 0.  One process per GPU (torchrun / torch.distributed.run; RCCL is torch's "nccl" backend).

The encoders and the video/text datasets are out of this build's scope, so the
runnable mode is `--synthetic`: seeded CLIP-shaped token features stand in for the encoder outputs
and the model runs in feature mode.  With real encoders, construct
`NeighborRetr(args, clip=<module with encode_text/encode_image/logit_scale>)` instead.

  python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 main_retrieval.py \\
      --do_train 1 --synthetic --batch_size 128 --max_words 24 --max_frames 12 --mb_batch 4 --epochs 1
"""
import argparse
import math
import os
import time

import numpy as np
import torch
import torch.distributed as dist


def get_args():
    p = argparse.ArgumentParser("NeighborRetr on MI355X")
    # loss parameters (args_parser.py:25-41)
    p.add_argument("--centrality_scale", default=0.3, type=float)
    p.add_argument("--kl_weight", default=1.0, type=float)
    p.add_argument("--uniform_weight", default=1.0, type=float)
    p.add_argument("--ot_temperature", default=0.1, type=float, help="parsed and unused, as in the reference")
    p.add_argument("--beta", default=0.7, type=float)
    p.add_argument("--num_neighbors", default=20, type=int)
    p.add_argument("--temperature", default=3.0, type=float)
    p.add_argument("--neighbor_weight", default=1.0, type=float)
    # data loading / modes / dataset (accepted for command-line compatibility)
    p.add_argument("--workers", default=8, type=int)
    p.add_argument("--pin_memory", action="store_true")
    p.add_argument("--prefetch_factor", default=4, type=int)
    p.add_argument("--persistent_workers", action="store_true")
    p.add_argument("--video_cache_size", default=64, type=int)
    p.add_argument("--use_prefetch", action="store_true")
    p.add_argument("--timeout", default=0, type=int)
    p.add_argument("--save_model", action="store_true")
    p.add_argument("--do_train", type=int, default=0)
    p.add_argument("--do_eval", type=int, default=0)
    p.add_argument("--detect_grad", action="store_true")
    p.add_argument("--datatype", default="msrvtt", type=str)
    p.add_argument("--anno_path", type=str, default="data/MSR-VTT/anno")
    p.add_argument("--video_path", type=str, default="data/MSR-VTT/videos")
    p.add_argument("--output_dir", default="output", type=str)
    p.add_argument("--seed", type=int, default=42)
    # optimisation
    p.add_argument("--lr", type=float, default=1e-4)
    p.add_argument("--coef_lr", type=float, default=1e-3)
    p.add_argument("--warmup_proportion", default=0.1, type=float)
    p.add_argument("--weight_decay", type=float, default=0.2)
    p.add_argument("--epochs", type=int, default=5)
    # batch
    p.add_argument("--batch_size", type=int, default=128, help="GLOBAL batch (data_dataloaders.py:38)")
    p.add_argument("--batch_size_val", type=int, default=128)
    p.add_argument("--memory_size", type=int, default=512, help="parsed and unused, as in the reference")
    p.add_argument("--mb_batch", type=int, default=10)
    p.add_argument("--max_words", type=int, default=24)
    p.add_argument("--max_frames", type=int, default=12)
    p.add_argument("--video_framerate", type=int, default=1)
    # distributed / model
    p.add_argument("--device", default="cpu", type=str)
    p.add_argument("--world_size", default=1, type=int)
    p.add_argument("--local_rank", "--local-rank", default=0, type=int)
    p.add_argument("--distributed", default=0, type=int)
    p.add_argument("--n_display", type=int, default=50)
    p.add_argument("--base_encoder", default="ViT-B/32", type=str)
    p.add_argument("--num_hidden_layers", type=int, default=4)
    p.add_argument("--init_model", default=None, type=str)
    # this build
    p.add_argument("--synthetic", action="store_true", help="seeded token features instead of encoders + datasets")
    p.add_argument("--synthetic_train", type=int, default=2048, help="synthetic training pairs")
    p.add_argument("--synthetic_test", type=int, default=1000, help="synthetic test pairs (MSR-VTT 1k-A size)")
    p.add_argument("--precision", default="bf16", choices=["bf16", "bf16x3", "bf16_all"])
    p.add_argument("--dist_backend", default="nccl", choices=["nccl", "gloo"],
                   help="collective backend: nccl = RCCL over xGMI (one GPU per rank); gloo only to rehearse several "
                        "ranks on ONE GPU (tests)")
    p.add_argument("--centrality_multi_token", default="raise", choices=["raise", "mean"],
                   help="several global tokens per sample (ActivityNet token counts): 'raise' like the reference "
                        "(until_module.py:321), 'mean' = centrality weight averaged over the sample's global tokens")
    p.add_argument("--encoders", type=int, default=0,
                   help="1: BASELINE configs[4] -- ViT-B/32 image tower, text tower and temporal transformer (stock "
                        "PyTorch-ROCm modules, random init unless --init_model) in front of the HIP head; --synthetic then "
                        "feeds random pixels [b, frames, 3, 224, 224] and token ids instead of token features")
    p.add_argument("--hubness_k", type=int, default=0,
                   help="k > 0 (at most 128): the evaluation also reports hubness of the top-k lists in both directions "
                        "(k-occurrence skewness, hubs, anti-hubs, bad hubs; DESIGN.md); 0 = off")
    p.add_argument("--test_norm", default="none", choices=["none", "is", "dsl", "qbnorm", "sinkhorn", "qbsinkhorn"],
                   help="test-time hubness reduction, reported next to the raw metrics: is (inverted softmax), dsl (dual "
                        "softmax), qbnorm (QB-Norm with the memory bank as querybank), sinkhorn (the model's own log-domain "
                        "Sinkhorn balancing on the test similarity), qbsinkhorn (its querybank form; DESIGN.md); none = off")
    p.add_argument("--test_norm_beta", type=float, default=20.0, help="inverse temperature beta of --test_norm")
    p.add_argument("--test_norm_iters", type=int, default=50,
                   help="--test_norm sinkhorn | qbsinkhorn: Sinkhorn iterations (the reference's num_iterations)")
    p.add_argument("--qb_k", type=int, default=1,
                   help="--test_norm qbnorm: a gallery item is active when it is in the top-qb_k list of some querybank item")
    p.add_argument("--local_scaling", default="none", choices=["none", "csls", "nicdm", "ls"],
                   help="local-scaling hubness reduction, reported next to the raw metrics: every score rescaled by statistics of "
                        "the two items' k-nearest neighbourhoods -- csls (minus the mean neighbour similarities), nicdm (distance "
                        "over the mean neighbour distances), ls (squared distance over the k-th neighbour distances; DESIGN.md); "
                        "none = off.  Not together with --test_norm")
    p.add_argument("--local_scaling_k", type=int, default=10, help="--local_scaling: neighbourhood size k (at most 128)")
    p.add_argument("--local_scaling_bank", type=int, default=0, choices=[0, 1],
                   help="--local_scaling: 1 takes the neighbourhoods in the memory bank (the querybank of --test_norm qbnorm) "
                        "instead of the test set")
    p.add_argument("--mutual_proximity", default="none", choices=["none", "emp", "gauss"],
                   help="mutual-proximity hubness reduction, reported next to the raw metrics: every score replaced by the "
                        "probability that it beats the scores of its text's line and of its video's line -- emp (the empirical "
                        "ranks, ties counted half), gauss (a normal fitted to each line; DESIGN.md); no temperature, no k; none = "
                        "off.  Not together with --test_norm or --local_scaling")
    p.add_argument("--mutual_proximity_bank", type=int, default=0, choices=[0, 1],
                   help="--mutual_proximity: 1 takes the lines in the memory bank (the querybank of --test_norm qbnorm) instead of "
                        "the test set")
    p.add_argument("--bootstrap", type=int, default=0,
                   help="N > 0: N bootstrap resamples of the test queries (the videos of a multi-sentence set) on the GPU: a percentile "
                        "confidence interval for every reported metric and, for a correction, a paired interval of its difference "
                        "to the raw ranking (DESIGN.md 6.7); at most 2^20; 0 = off")
    p.add_argument("--bootstrap_seed", type=int, default=0,
                   help="--bootstrap: seed of the counter-based draws (text->video uses it, video->text seed + 1)")
    p.add_argument("--bootstrap_level", type=float, default=0.95, help="--bootstrap: coverage of the intervals, in (0, 1)")
    p.add_argument("--ir_metrics", type=int, default=0, choices=[0, 1],
                   help="1: the rank-aware IR metrics MRR, mAP, nDCG@10 and R-precision of every relevant (text, video) pair in both "
                        "directions, next to R@K, for the raw ranking and for a correction; with --bootstrap their intervals too "
                        "(DESIGN.md 6.8); 0 = off")
    p.add_argument("--permutation", type=int, default=0,
                   help="N > 0: a paired permutation (randomisation) test with N relabellings on the GPU: for a correction, is it "
                        "significantly better than the raw ranking; with --compare_model, is this model better than that one: the "
                        "difference of every metric with its two-sided p-value (DESIGN.md 6.10); at most 2^20; 0 = off")
    p.add_argument("--permutation_seed", type=int, default=0,
                   help="--permutation: seed of the counter-based swap bits (text->video uses it, video->text seed + 1)")
    p.add_argument("--compare_model", default=None, type=str, metavar="PATH",
                   help="--do_eval with --permutation N: the test set is scored again with the same architecture loaded from PATH, and "
                        "'model - compared' lines give the paired permutation test (with --bootstrap the paired interval too) of "
                        "this model against it")
    p.add_argument("--hubness_test", type=int, default=0, choices=[0, 1],
                   help="1, with --hubness_k K and --permutation N: the paired permutation test of the hubness figures (skewness, "
                        "hubs, bad hubs, anti-hubs, ...) from the relabelled top-K lists on the GPU, for a correction against raw, "
                        "with --compare_model and for the EMA: every difference with its two-sided p-value (DESIGN.md 6.13); 0 = off")
    p.add_argument("--rerank_top", type=int, default=0, metavar="C",
                   help="two-stage retrieval after the exhaustive evaluation: a pooled single-vector prefilter picks C candidates "
                        "per query, the token-level score re-ranks those only; logs R@K and the candidate recall per direction "
                        "(DESIGN.md 6.14); 1..128; 0 = off")
    p.add_argument("--rerank_norm", default="none", choices=["none", "is", "qbnorm"],
                   help="with --rerank_top C: the candidate scores are also normalised against the memory bank as querybank -- is "
                        "(every query) or qbnorm (the queries whose top-1 candidate is in the bank's activation set) -- with "
                        "--test_norm_beta and --qb_k; the statistics are computed once per gallery, one fused launch normalises "
                        "and re-ranks the lists; logs R@K, candidate recall and the gated share per direction and, with "
                        "--hubness_k K <= C, the hubness of the two-stage lists before and after (DESIGN.md 6.15); none = off")
    p.add_argument("--rerank_local_scaling", default="none", choices=["none", "csls", "nicdm", "ls"],
                   help="with --rerank_top C: the candidate scores are also locally scaled (CSLS, NICDM or LS) -- every gallery "
                        "item's neighbourhood is taken once per gallery in the memory bank as querybank, a query's among its own "
                        "candidates; one fused launch corrects and re-ranks the lists; logs R@K and candidate recall per direction "
                        "and, with --hubness_k K <= C, the hubness of the two-stage lists before and after (DESIGN.md 6.17); not "
                        "with --rerank_norm; none = off")
    p.add_argument("--rerank_local_scaling_k", type=int, default=10, metavar="K",
                   help="with --rerank_local_scaling: the neighbourhood size, 1..--rerank_top")
    p.add_argument("--rerank_mutual_proximity", default="none", choices=["none", "emp", "gauss"],
                   help="with --rerank_top C: the candidate scores are also replaced by their mutual proximity (empirical counts or "
                        "the Gaussian model; no temperature, no k) -- every gallery item's line of scores is taken once per gallery "
                        "in the memory bank as querybank, a query's among its own candidates; one fused launch corrects and re-ranks "
                        "the lists; logs R@K and candidate recall per direction and, with --hubness_k K <= C, the hubness of the "
                        "two-stage lists before and after (DESIGN.md 6.18); not with --rerank_norm or --rerank_local_scaling; "
                        "none = off")
    p.add_argument("--rerank_lists", type=int, default=0, metavar="L",
                   help="with --rerank_top C: the prefilter goes through an inverted file of L k-means lists over each gallery's "
                        "pooled vectors and scores a query against its --rerank_probe closest lists only; logs the two-stage "
                        "figures of those candidates, the mean pool size and the share of the exact prefilter's candidates kept "
                        "(DESIGN.md 6.16); 0 = off, the exact prefilter")
    p.add_argument("--rerank_probe", type=int, default=0, metavar="P",
                   help="with --rerank_lists L: the lists a query scans, 1..min(L, 128)")
    p.add_argument("--rerank_ivf_iters", type=int, default=10, help="with --rerank_lists: k-means rounds of the index build (>= 0)")
    p.add_argument("--rerank_ivf_seed", type=int, default=0, help="with --rerank_lists: seed of the initial centroids")
    p.add_argument("--hip_graph", type=int, default=0,
                   help="1: the training step replayed from captured HIP graphs instead of ~90 eager launches.  One rank: forward + "
                        "backward as ONE graph.  Several ranks: the whole data-parallel step -- exchange, loss, backward, gradient "
                        "average -- as one graph with the RCCL collectives inside, or (when that is refused / fails its validation, "
                        "and on gloo) the rank-local segments between the collectives as graphs; the ranks decide together")
    p.add_argument("--optimizer", default="adamw", choices=["adamw", "bertadam"],
                   help="adamw: torch.optim.AdamW at --lr on every tensor.  bertadam: the reference's optimizer and grouping "
                        "(training/optimizer.py: `clip.` names at lr * coef_lr, no decay on bias / LayerNorm, warm-up + cosine "
                        "over len(train) * epochs steps) as multi-tensor HIP kernels, with the trainer's global clip and "
                        "logit-scale clamp inside; under --hip_graph 1 on one rank the update is part of the replayed graph")
    p.add_argument("--skip_nonfinite", type=int, default=0, choices=[0, 1],
                   help="1: a training step whose gradients are not all finite (one undecodable video gives an all-zero mask and "
                        "NaN losses) updates nothing and is counted (DESIGN.md 6.9).  --optimizer bertadam decides on the device "
                        "inside its three launches -- no synchronisation, also inside the replayed graph -- and logs skips and "
                        "gradient norms at every --n_display line; --optimizer adamw tests the norm clip_grad_norm_ returns on "
                        "the host, which costs one synchronisation per step, with this flag only; 0 = off")
    p.add_argument("--ema_decay", type=float, default=0.0,
                   help="D in (0, 1): an exponential moving average of the weights with decay D, updated on the device after "
                        "every update that happened (DESIGN.md 6.11): inside the optimizer's launches with --optimizer bertadam "
                        "(so inside the replayed graph and under --skip_nonfinite 1), two launches after optimizer.step() with "
                        "adamw.  Every epoch is evaluated a second time with the average (lines tagged EMA) and, with "
                        "--save_model, saved as pytorch_model_ema.bin.N, which --init_model / --compare_model load; 0 = off")
    p.add_argument("--ema_warmup", type=int, default=1, choices=[0, 1],
                   help="--ema_decay: 1 ramps the decay up as min(D, (1 + n) / (10 + n)) over the first updates; 0 uses D throughout")
    p.add_argument("--synthetic_blank", default="", metavar="STEP[:RANK]",
                   help="--synthetic: in global step STEP (1-based) the first video of the batch of rank RANK (default 0) comes "
                        "back the way the reference's loader returns an undecodable one, all zeros with an all-zero mask")
    p.add_argument("--save_state_every", type=int, default=0, metavar="N",
                   help="N > 0: after every N-th global step and at the end of every epoch rank 0 writes the whole training state "
                        "(weights, raw memory-bank ring, noise stream, optimizer with its device counters and guard, EMA; "
                        "DESIGN.md 6.12) to <output_dir>/training_state.pt, atomically; 0 = off")
    p.add_argument("--resume", default=None, metavar="PATH|auto",
                   help="continue training from a training-state file, bit for bit, also in the middle of an epoch and under "
                        "--hip_graph 1; auto: <output_dir>/training_state.pt when it exists, a fresh start otherwise")
    p.add_argument("--max_steps", type=int, default=0, metavar="N",
                   help="N > 0: training stops after global step N, having written the training state (a time-boxed job); 0 = none")
    args = p.parse_args()
    if args.save_state_every < 0 or args.max_steps < 0:
        p.error("--save_state_every and --max_steps must be >= 0")
    if args.resume is not None and not args.do_train:
        p.error("--resume continues training: it needs --do_train 1")
    if args.resume is not None and args.init_model:
        p.error("--resume restores the weights itself: not together with --init_model")
    try:
        blank = [int(v) for v in args.synthetic_blank.split(":")] if args.synthetic_blank else [0, 0]
        args.blank_step, args.blank_rank = blank if len(blank) == 2 else (blank[0], 0)
    except ValueError:
        p.error("--synthetic_blank takes STEP or STEP:RANK")
    if args.test_norm_iters < 1:
        p.error("--test_norm_iters must be >= 1")
    if args.local_scaling != "none" and args.test_norm != "none":
        p.error("--local_scaling and --test_norm are separate corrections: choose one of them")
    if args.mutual_proximity != "none" and args.test_norm != "none":
        p.error("--mutual_proximity and --test_norm are separate corrections: choose one of them")
    if args.mutual_proximity != "none" and args.local_scaling != "none":
        p.error("--mutual_proximity and --local_scaling are separate corrections: choose one of them")
    if not 1 <= args.local_scaling_k <= 128:
        p.error("--local_scaling_k must lie in [1, 128]")
    if not 0 <= args.bootstrap <= 1 << 20:
        p.error("--bootstrap must lie in [0, 2^20]")
    if not 0 <= args.bootstrap_seed < (1 << 64) - 1:
        p.error("--bootstrap_seed must lie in [0, 2^64 - 1)")
    if not 0.0 < args.bootstrap_level < 1.0:
        p.error("--bootstrap_level must lie in (0, 1)")
    if not 0 <= args.permutation <= 1 << 20:
        p.error("--permutation must lie in [0, 2^20]")
    if not 0 <= args.permutation_seed < (1 << 64) - 1:
        p.error("--permutation_seed must lie in [0, 2^64 - 1)")
    if not (args.ema_decay == 0.0 or 0.0 < args.ema_decay < 1.0):
        p.error("--ema_decay must be 0 (off) or lie in (0, 1)")
    if args.ema_decay and not args.do_train:
        p.error("--ema_decay belongs to training (--do_train 1); evaluate a saved average with --init_model")
    if args.compare_model and not (args.do_eval and not args.do_train and args.permutation > 0):
        p.error("--compare_model works with --do_eval (without --do_train) and needs --permutation > 0")
    corrected = args.test_norm != "none" or args.local_scaling != "none" or args.mutual_proximity != "none"
    if args.permutation and not (corrected or args.compare_model or args.ema_decay):
        p.error("--permutation needs a correction (--test_norm, --local_scaling, --mutual_proximity), --compare_model or "
                "--ema_decay: there is nothing to compare")
    if not 0 <= args.rerank_top <= 128:
        p.error("--rerank_top must lie in [0, 128] (0 = off)")
    if args.rerank_norm != "none" and args.rerank_top < 1:
        p.error("--rerank_norm normalises candidate lists: it needs --rerank_top >= 1")
    if args.rerank_local_scaling != "none":
        if args.rerank_norm != "none":
            p.error("--rerank_local_scaling and --rerank_norm both correct the candidate scores: choose one")
        if not 1 <= args.rerank_local_scaling_k <= 128:
            p.error("--rerank_local_scaling_k must lie in [1, 128]")
        if args.rerank_top < args.rerank_local_scaling_k:
            p.error(f"--rerank_local_scaling takes a query's neighbourhood among its candidates: it needs --rerank_top >= "
                    f"--rerank_local_scaling_k = {args.rerank_local_scaling_k}")
    if args.rerank_mutual_proximity != "none":
        for flag, value in (("--rerank_norm", args.rerank_norm), ("--rerank_local_scaling", args.rerank_local_scaling)):
            if value != "none":
                p.error(f"--rerank_mutual_proximity and {flag} both correct the candidate scores: choose one")
        if args.rerank_top < 1:
            p.error("--rerank_mutual_proximity corrects candidate lists: it needs --rerank_top >= 1")
    if args.rerank_lists < 0:
        p.error("--rerank_lists must be >= 0 (0 = off)")
    if args.rerank_lists and args.rerank_top < 1:
        p.error("--rerank_lists restricts the prefilter of two-stage retrieval: it needs --rerank_top >= 1")
    if args.rerank_lists and not 1 <= args.rerank_probe <= min(args.rerank_lists, 128):
        p.error(f"--rerank_probe must lie in [1, min(--rerank_lists, 128) = {min(args.rerank_lists, 128)}]")
    if not args.rerank_lists and args.rerank_probe:
        p.error("--rerank_probe needs --rerank_lists >= 1")
    if args.rerank_ivf_iters < 0:
        p.error("--rerank_ivf_iters must be >= 0")
    if args.hubness_test and not (args.hubness_k > 0 and args.permutation > 0):
        p.error("--hubness_test needs --hubness_k > 0 and --permutation > 0")
    if args.batch_size % max(1, int(os.environ.get("WORLD_SIZE", "1"))):
        raise ValueError("--batch_size must divide over the ranks (args_parser.py:149-165)")
    return args


def setup_distributed(args):
    """One process per GPU; rendezvous from the torchrun environment (setup.py:44-69)."""
    args.world_size = int(os.environ.get("WORLD_SIZE", "1"))
    args.rank = int(os.environ.get("RANK", "0"))
    args.local_rank = int(os.environ.get("LOCAL_RANK", str(args.local_rank)))
    if not torch.cuda.is_available():
        raise RuntimeError("the HIP path needs an MI355X; there is no CPU fallback")
    n_dev = torch.cuda.device_count()
    if args.dist_backend == "nccl" and args.local_rank >= n_dev:
        raise RuntimeError(f"LOCAL_RANK {args.local_rank} but {n_dev} GPU(s) visible: RCCL needs one GPU per rank")
    args.device_index = args.local_rank % n_dev                     # gloo rehearsal: ranks share the card
    torch.cuda.set_device(args.device_index)
    args.device = torch.device("cuda", args.device_index)
    if args.world_size > 1:
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=args.device)  # "nccl" is RCCL on ROCm
        else:
            dist.init_process_group("gloo")
    # AllGather / packed_allgather slice gradients by GLOBAL rank
    args.local_rank = args.rank
    return args


def log(args, msg):
    if args.rank == 0:
        print(time.strftime("%H:%M:%S"), msg, flush=True)


def _tagged_log(tag):
    """log, or with a tag a log that puts the tag in front of every message."""
    return log if not tag else (lambda args, msg: log(args, f"{tag} {msg}"))


class SyntheticFeatures:
    """Per-rank shard of seeded (text, video) token features: the encoders' stand-in."""

    def __init__(self, args, n, stream, seed):
        from neighborretr_amd import synth
        t, v, tm, vm = synth.make_samples(seed, stream, n, args.max_words, args.max_frames)
        self.t, self.v, self.tm, self.vm = (torch.from_numpy(a) for a in (t, v, tm, vm))
        self.n = n
        self.b = args.batch_size // args.world_size
        self.W, self.rank, self.B = args.world_size, args.rank, args.batch_size

    def __len__(self):
        return self.n // self.B

    def batch(self, i, device):
        lo = i * self.B + self.rank * self.b
        sl = slice(lo, lo + self.b)
        idx = torch.arange(lo, lo + self.b)
        return tuple(x.to(device, non_blocking=True) for x in (self.t[sl], self.tm[sl], self.v[sl], self.vm[sl], idx))


class SyntheticClips:
    """Per-rank shard of seeded raw inputs for --encoders 1: token ids [b, Nt] (EOT at the end of the mask) and pixels
    [b, Nv, 3, 224, 224], generated on the device batch by batch (a whole epoch of frames would not fit the host)."""

    def __init__(self, args, n, stream, seed, resolution=224):
        from neighborretr_amd import synth
        from neighborretr_amd.encoders import synthetic_text_ids
        _, _, tm, vm = synth.make_samples(seed, stream, n, args.max_words, args.max_frames, d=8)
        self.tm, self.vm = torch.from_numpy(tm), torch.from_numpy(vm)
        self.ids = synthetic_text_ids(self.tm, seed=seed)
        self.n, self.res, self.seed = n, resolution, seed
        self.b = args.batch_size // args.world_size
        self.W, self.rank, self.B = args.world_size, args.rank, args.batch_size

    def __len__(self):
        return self.n // self.B

    def rows(self, index, device):
        g = torch.Generator(device=device).manual_seed(self.seed * 1000003 + int(index[0]))
        video = torch.randn((len(index), self.vm.shape[1], 3, self.res, self.res), generator=g, device=device)
        return (self.ids[index].to(device), self.tm[index].to(device), video, self.vm[index].to(device), index.to(device))

    def batch(self, i, device):
        lo = i * self.B + self.rank * self.b
        return self.rows(torch.arange(lo, lo + self.b), device)


def encode(model, batch):
    """(text_feat, text_mask, video_feat, video_mask, idx) of a raw batch: the encoders' outputs, or the inputs themselves
    in feature mode."""
    text, tm, video, vm, idx = batch
    if model.feature_mode:
        return batch
    with torch.no_grad():
        tf, vf = model.get_text_video_feat(text, tm, video, vm)
    return tf, tm, vf, vm, idx


def load_memory_bank(args, model, data):
    """memory_bank.py:80-229: run mb_batch batches through the (feature-mode) encoders under no_grad,
    gather them over the ranks, hand them to the model as plain attributes."""
    from neighborretr_amd.dist import packed_allgather
    n = min(args.mb_batch, len(data))
    was_training = model.training
    model.eval()                                            # memory_bank.py:102
    feats = [encode(model, data.batch(i, args.device)) for i in range(n)]
    model.train(was_training)
    with torch.no_grad():
        tf, tm, vf, vm, idx = (torch.cat([f[k] for f in feats], 0) for k in range(5))
        tf, vf, idx, tm, vm = packed_allgather(tf, vf, idx, tm, vm, args)
    model.mb_ind, model.mb_feat_t, model.mb_feat_v = idx, tf.contiguous(), vf.contiguous()
    model.mb_mask_t, model.mb_mask_v, model.mb_batch = tm.contiguous(), vm.contiguous(), tf.shape[0]   # memory_bank.py:211
    log(args, f"memory bank: {tf.shape[0]} samples ({n} batches x {args.batch_size})")
    return tf.shape[0]


def clear_memory_bank(model):
    model._init_memory_bank()


class GraphedStep:
    """Forward + backward of one training step as a captured HIP graph with static input buffers: run() leaves the losses in
    .losses and the gradients in the parameters' .grad.  Without `optimizer` the optimizer step stays eager and with the caller.

    optimizer (a neighborretr_amd.optim.BertAdam): the update belongs to the step.  One rank: its three launches are captured
    behind the backward, so one replay = forward + backward + update (the table of pointers the kernels read is filled by a
    copy node from a pinned host buffer the optimizer keeps: the static gradients only come into being inside the capture).
    Several ranks: the same launches follow the step's replay, after the gradient average, outside the forms that
    CollectiveCapture validates.  Warm-up passes and re-captures apply no update; a batch of another shape takes an eager step
    that ends in optimizer.step().  Either way run() returns with the update issued, and the optimizer's step count is the
    number of run() calls.

    An optimizer built with skip_nonfinite=True keeps its place: on one rank its guarded launches are captured behind the
    backward, where issue() is captured, and they record the step's five losses from a [5] tensor stacked inside the capture
    (static, so its address can be baked in).  On several ranks they follow the replay, after the gradient average: every rank
    then holds the same flat gradient, takes the same decision and stays in step with the others; the losses each rank records
    are its own.  The optimizer's step count is then the number of run() calls minus the steps the device skipped.

    world_size > 1: the step that is replayed is the WHOLE data-parallel step -- exchange step, loss, backward with the
    reductions of its differentiable collectives, and the gradient average over the ranks (one all-reduce of a flat buffer that
    the parameters' .grad are views of; what DistributedDataParallel's bucketed all-reduce computes, optimizer.py:79-84) --
    in the best form every rank can take (neighborretr_amd.comm.CollectiveCapture): ONE graph with the RCCL collectives
    inside; else the rank-local segments between the collectives as graphs (comm.SegmentedStep); else eager launches.  Each
    form is validated against the eager step on every rank before it is used."""

    def __init__(self, model, example, params, args=None, optimizer=None):
        self.static = [t.clone() for t in example]
        self.params = params
        self.model = model
        self.optimizer = optimizer
        if optimizer is not None:
            from neighborretr_amd.optim import BertAdam
            if not isinstance(optimizer, BertAdam):
                raise TypeError("GraphedStep(optimizer=...) takes a neighborretr_amd.optim.BertAdam: its step is three capturable "
                                f"launches; got {type(optimizer).__name__}")
        self.world = int(getattr(args, "world_size", 1)) if args is not None else 1
        self.rank = int(getattr(args, "rank", 0)) if args is not None else 0
        self.backend = getattr(args, "dist_backend", "nccl") if args is not None else "nccl"
        self.form = "eager"
        self.cc = None
        self.capture()

    def capture(self):
        with self.model.graph_capture_mode():
            if self.world > 1:
                self._capture_parallel()
            else:
                self._capture()

    def _warm_up(self, step):
        """Warm-up on a side stream, as graph capture requires -- with the bank FROZEN: a warm-up step that pushed its batch
        would leave the static batch in the bank three times (and three more times after every re-capture), which is not the
        reference's FIFO (modeling.py:222-249)."""
        model = self.model
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        model.bank_frozen = True
        try:
            with torch.cuda.stream(side):
                for _ in range(3):
                    step()
        finally:
            model.bank_frozen = False
        torch.cuda.current_stream().wait_stream(side)

    def _capture(self):
        model, params = self.model, self.params
        B = self.static[0].shape[0]

        def fwd_bwd():
            return torch.autograd.grad(model(*self.static, 0)[0], params, allow_unused=True)
        self._warm_up(fwd_bwd)
        # the device-resident ring head must exist before the capture (creating it is a host-to-device copy)
        model._ring_ready(B)
        if self.optimizer is not None:
            self.optimizer.prepare(params, owner=self)   # moments, counters, workspace: allocated (and zeroed) outside the capture
        torch.cuda.synchronize()
        for p in params:
            p.grad = None
        # derived weights (bf16 hi/lo splits) are cached per parameter version: drop the caches so that the splits are
        # captured too and every replay re-derives them from the fp32 parameters the optimizer has just updated
        model._scorer_cache.clear()
        model._ctm_cache.clear()
        # torch.autograd.grad, not .backward(): the gradients come back as the graph's own static tensors and NO AccumulateGrad
        # node takes part.  Those nodes outlive a step whenever anything still holds its losses (a training loop's `losses`
        # variable, DDP), on the stream they were created on; a capture that has to synchronise with such a stream -- the
        # default stream in particular -- dies inside the runtime (PyTorch warns "AccumulateGrad node's stream does not match
        # ... break CUDA graph capture"; measured: tools/rank_local_times.py, round 4).
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            losses = model(*self.static, 0)
            grads = torch.autograd.grad(losses[0], params, allow_unused=True)
            if self.optimizer is not None:
                for p, g in zip(params, grads):
                    p.grad = g
                if self.optimizer.skip_nonfinite:
                    self.optimizer.watch_losses(torch.stack([l.detach().float() for l in losses]))
                self._updated = self.optimizer.issue()           # captured, not executed: advance() follows every replay
        self.losses = tuple(l.detach() for l in losses)          # the loss VALUES only (no autograd graph kept alive)
        del losses
        self.grads = list(grads)                     # static gradient buffers of the graph (None: the step does not reach it)
        self.replay, self.form = self.graph.replay, "whole"
        self._remember_bank()

    def _remember_bank(self):
        # What the graph has baked in: the addresses of the five bank tensors and of the device ring head.  Hold
        # strong references (a bank replaced from outside must not hand its blocks to somebody else while this graph
        # can still replay) and remember the bank's storage generation; run() re-captures when it has moved on.
        model = self.model
        self.bank_refs = (dict(model._mb), model._mb_head_dev)
        self.generation = model._mb_gen

    def _capture_parallel(self):
        from neighborretr_amd import comm
        model, params, W = self.model, self.params, self.world
        B = self.static[0].shape[0] * W
        if self.cc is None:
            self.cc = comm.CollectiveCapture(W, self.rank, log=lambda msg: print(f"[GraphedStep] {msg}", flush=True))

        seen = {}

        def fwd_bwd():
            seen["g"] = torch.autograd.grad(model(*self.static, 0)[0], params, allow_unused=True)
        self._warm_up(fwd_bwd)
        model._ring_ready(B)
        torch.cuda.synchronize()
        # the parameters that receive a gradient (the same set in every step: DDP's find_unused_parameters bookkeeping,
        # optimizer.py:79-84, done once) get views of ONE flat buffer as their .grad
        used = [p for p, g in zip(params, seen.pop("g")) if g is not None]
        flat = torch.zeros(sum(p.numel() for p in used), dtype=torch.float32, device=used[0].device)
        views, off = [], 0
        for p in used:
            views.append(flat[off:off + p.numel()].view_as(p))
            off += p.numel()
        out = {}
        rng = model._rng_state_on(flat.device)

        def step():
            losses = model(*self.static, 0)
            grads = torch.autograd.grad(losses[0], used)          # (no AccumulateGrad nodes in a captured step: see _capture)
            torch._foreach_copy_(views, list(grads))
            comm.all_reduce(flat)                     # the gradient average over the ranks: one collective, one flat buffer
            flat.mul_(1.0 / W)
            out["losses"] = torch.stack([l.detach() for l in losses])

        def eager_pass():
            rng[1] = 4242                             # the same DPC-KNN tie-break draws for the eager and the replayed pass
            step()

        def result():
            return [out["losses"], flat]

        def same(a, b_):
            return bool(torch.allclose(a[0], b_[0], rtol=1e-4, atol=1e-6)
                        and (a[1] - b_[1]).norm() <= 1e-3 * b_[1].norm() + 1e-12)

        def whole():
            model._scorer_cache.clear()
            model._ctm_cache.clear()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                step()

            def replay_pass():
                rng[1] = 4242
                g.replay()
            return replay_pass, g

        def segmented():
            model._scorer_cache.clear()
            model._ctm_cache.clear()
            seg = comm.SegmentedStep(step, capture_error_mode="relaxed").capture()

            def replay_pass():
                rng[1] = 4242
                seg.replay()
            return replay_pass, seg
        freeze = lambda on: setattr(model, "bank_frozen", on)      # noqa: E731
        # the validation passes pin the DPC-KNN noise counter to one value; the run continues from where it stood before them
        # (otherwise every re-capture -- one per epoch -- restarts the same noise sequence and a --hip_graph 1 run diverges
        # from the eager run with the same seed)
        rng_before = rng.clone()
        form = self.cc.attempt("whole-step", eager_pass, whole, result, same, freeze) if self.backend == "nccl" else None
        self.form = "whole"
        if form is None:
            form = self.cc.attempt("segmented", eager_pass, segmented, result, same, freeze)
            self.form = "segmented"
        rng.copy_(rng_before)
        if form is None:
            self.form, self.replay, self.keep = "eager", step, None
        else:
            self.keep = form[1]
            self.replay = form[1].replay
        self.grads = None
        self._used, self._views, self._out = used, views, out
        self._remember_bank()

    def _eager(self, batch):
        """A batch whose shapes differ from the captured ones (a loader's last, shorter batch): one eager step with the same
        outcome -- losses returned, gradients left in .grad -- instead of a graph per shape."""
        if self.world > 1:
            raise ValueError("GraphedStep on several ranks needs batches of one shape (the exchange step gathers equal shards: drop "
                             f"the loader's last batch); got {[tuple(t.shape) for t in batch]} after {[tuple(t.shape) for t in self.static]}")
        losses = self.model(*batch, 0)
        grads = torch.autograd.grad(losses[0], self.params, allow_unused=True)
        for p, g in zip(self.params, grads):
            p.grad = g
        if self.optimizer is not None:
            if self.optimizer.skip_nonfinite:
                self.optimizer.watch_losses(torch.stack([l.detach().float() for l in losses]))
            self.optimizer.step()
        return tuple(l.detach() for l in losses)

    def run(self, batch):
        if any(tuple(src.shape) != tuple(dst.shape) for dst, src in zip(self.static, batch)):
            return self._eager(batch)
        if self.model._mb_gen != self.generation:    # the bank's tensors / ring head were replaced: the graph is stale
            self.capture()
        for dst, src in zip(self.static, batch):
            dst.copy_(src)
        self.replay()
        if self.world > 1:
            for p, g in zip(self._used, self._views):    # optimizer.zero_grad(set_to_none=True) drops them: put them back
                p.grad = g
            if self.optimizer is not None:
                if self.optimizer.skip_nonfinite:
                    self.optimizer.watch_losses(self._out["losses"].float())
                self.optimizer.step()                    # the same table every step: the views never move
            return tuple(self._out["losses"].unbind(0))
        for p, g in zip(self.params, self.grads):    # optimizer.zero_grad(set_to_none=True) drops them: put them back
            p.grad = g
        if self.optimizer is not None:
            self.optimizer.advance(self._updated)        # the replay has applied the update: versions and the step mirror
        return self.losses


class StateKeeper:
    """--save_state_every / --max_steps / --resume: writes <output_dir>/training_state.pt on rank 0 and prints
    every rank's digest line.  Epochs and steps count from 0 here, as in the state's position."""

    def __init__(self, args, model, optimizer, ema):
        self.args, self.model, self.optimizer, self.ema = args, model, optimizer, ema
        self.path = os.path.join(args.output_dir, "training_state.pt")
        self.stopped = False

    def capture(self, epoch, next_step, global_step):
        from neighborretr_amd import checkpoint
        return checkpoint.capture_state(self.model, self.optimizer, self.ema,
                                        position=dict(epoch=epoch, next_step=next_step, global_step=global_step),
                                        config=checkpoint.config_from_args(self.args),
                                        host_guard=getattr(self.args, "_host_skips", None))

    def write(self, state):
        from neighborretr_amd import checkpoint
        if self.args.rank == 0:
            checkpoint.save(self.path, state)
            pos = state["position"]
            log(self.args, f"training state written: epoch {pos['epoch'] + 1}, next step {pos['next_step'] + 1} "
                           f"(global step {pos['global_step']}) -> {self.path}")

    def digest_line(self, state, epoch):
        from neighborretr_amd import checkpoint
        print(f"rank {self.args.rank} epoch {epoch + 1} training state sha256 {checkpoint.digest(state)[:16]}", flush=True)

    def after_step(self, epoch, i, global_step):
        """After step i of `epoch`: the N-th step's write, and the stop of --max_steps (state written, digest line) -> stop."""
        args = self.args
        stop = bool(args.max_steps) and global_step >= args.max_steps
        due = bool(args.save_state_every) and global_step % args.save_state_every == 0
        if stop or (due and args.rank == 0):
            state = self.capture(epoch, i + 1, global_step)
            self.write(state)
            if stop:
                self.digest_line(state, epoch)
        self.stopped = stop
        return stop

    def end_of_epoch(self, epoch, global_step):
        """After the epoch's evaluation, saved models and EMA pass: position (epoch + 1, 0), so a resume re-runs none of them."""
        state = self.capture(epoch + 1, 0, global_step)
        if self.args.save_state_every:
            self.write(state)
        self.digest_line(state, epoch)


def resume_training(args, state, keeper):
    """--resume: the loaded state into the run's model, optimizer and EMA on every rank -> its position.  Several ranks compare
    the digests of what they hold afterwards with one all-gather of the 32 bytes; a difference raises on every rank."""
    from neighborretr_amd import checkpoint
    if args.skip_nonfinite and args.optimizer != "bertadam":
        args._host_skips = dict(skipped=0, consecutive=0, max_consecutive=0, norms=[])
    pos = checkpoint.restore_state(state, keeper.model, keeper.optimizer, keeper.ema, host_guard=getattr(args, "_host_skips", None))
    if args.world_size > 1:
        mine = bytes.fromhex(checkpoint.digest(keeper.capture(**pos)))
        where = args.device if args.dist_backend == "nccl" else "cpu"
        got = [torch.empty(32, dtype=torch.uint8, device=where) for _ in range(args.world_size)]
        dist.all_gather(got, torch.tensor(list(mine), dtype=torch.uint8, device=where))
        seen = [bytes(g.cpu().tolist()).hex()[:16] for g in got]
        if len(set(seen)) != 1:
            raise RuntimeError(f"--resume: the ranks hold different training states after restoring: {seen}")
    log(args, f"resumed at epoch {pos['epoch'] + 1}, step {pos['next_step'] + 1} (global step {pos['global_step']})")
    return pos


def train_epoch(args, model, ddp, data, optimizer, epoch, global_step, ema=None, start=0, keeper=None):
    """ema: the run's WeightEma.  --optimizer bertadam drives it from its own launches; after an AdamW step that happened it
    takes its stand-alone update here.  start: the first step of this epoch to run (a resumed run; the memory bank is then the
    restored one); keeper: the run's StateKeeper, asked after every step."""
    from neighborretr_amd.dist import reduce_losses
    model.train()
    t0 = time.time()
    graphed = getattr(args, "_graphed_step", None)
    fused = args.optimizer == "bertadam"             # global clip, update and logit-scale clamp in the optimizer's kernels
    guard = bool(getattr(args, "skip_nonfinite", 0))
    if guard and not fused and not hasattr(args, "_host_skips"):
        args._host_skips = dict(skipped=0, consecutive=0, max_consecutive=0, norms=[])
    bank_steps = -(-int(getattr(model, "mb_batch", 0)) // args.batch_size)        # steps until a batch has left the memory bank
    warned = 0
    for i in range(start, len(data)):
        global_step += 1
        text, text_mask, video, video_mask, idx = data.batch(i, args.device)
        if global_step == getattr(args, "blank_step", 0) and args.rank == getattr(args, "blank_rank", 0):
            video, video_mask = video.clone(), video_mask.clone()   # dataloader_retrieval.py:278-315 after a failed decode
            video[0] = 0
            video_mask[0] = 0
        if args.hip_graph:
            if graphed is None:
                # a run resumed inside an epoch captures here, where the uninterrupted run replays: what the capture's warm-up
                # passes move is put back, so that the loaded state is the state this step starts from
                kept = None
                if start > 0:
                    from neighborretr_amd import checkpoint
                    kept = checkpoint.volatile_words(model)
                graphed = args._graphed_step = GraphedStep(model, (text, text_mask, video, video_mask, idx),
                                                           [p for p in model.parameters() if p.requires_grad], args,
                                                           optimizer=optimizer if fused else None)
                if kept is not None:
                    checkpoint.reapply_volatile(model, kept)
                log(args, f"training step replayed as: {graphed.form}")
            losses = graphed.run((text, text_mask, video, video_mask, idx))
            loss = None
        else:
            losses = ddp(text, text_mask, video, video_mask, idx, global_step)
            loss = losses[0]
            loss.backward()
        if fused:
            if not args.hip_graph:                   # (a graphed step has issued the update itself)
                if guard:
                    optimizer.watch_losses(torch.stack([l.detach().float() for l in losses]))
                optimizer.step()
            optimizer.zero_grad(set_to_none=True)
        else:
            norm = torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
            if guard:                                # the host's form of the guard: float() waits for the device, every step
                norm, hs = float(norm), args._host_skips
                hs["norms"].append(norm)
                del hs["norms"][:-max(args.n_display, 1)]             # the log line's window, no more
                if math.isfinite(norm):
                    hs["consecutive"] = 0
                    optimizer.step()
                    if ema is not None:
                        ema.update()
                else:
                    hs["skipped"] += 1
                    hs["consecutive"] += 1
                    hs["max_consecutive"] = max(hs["max_consecutive"], hs["consecutive"])
            else:
                optimizer.step()
                if ema is not None:
                    ema.update()
            optimizer.zero_grad(set_to_none=True)
            torch.clamp_(model.clip.logit_scale.data, max=float(np.log(100)))    # trainer.py:114-119
        if global_step % args.n_display == 0 or i == len(data) - 1:
            red = reduce_losses(losses, args).tolist()                            # one reduce instead of five
            lr = f" lr {optimizer.group_lr(applied=True)[1]:.3e}" if fused else ""     # the head's (decayed, non-CLIP) group, this step
            tail = ""
            if guard:
                window = min(args.n_display, i + 1)          # the steps since the last line (the records' window)
                stats, norms = _guard_report(args, optimizer, fused, window)
                finite = [v for v in norms if math.isfinite(v)]
                tail = (f" skipped {stats['skipped']} longest run {stats['max_consecutive']} grad norm median "
                        f"{float(np.median(finite)) if finite else float('nan'):.3e} max {max(finite) if finite else float('nan'):.3e}")
                if stats["consecutive"] > max(bank_steps, 0) and stats["consecutive"] > warned:
                    log(args, f"WARNING: {stats['consecutive']} training steps in a row had non-finite gradients and were skipped, "
                              f"more than the {bank_steps} steps a batch stays in the memory bank: the guard does not filter the "
                              "bank, look at the data")
                warned = stats["consecutive"]
            log(args, f"epoch {epoch} step {i + 1}/{len(data)} loss {red[0]:.4f} centrality {red[1]:.4f} "
                      f"uniform {red[2]:.4f} neighbor {red[3]:.4f} kl {red[4]:.4f}{lr} "
                      f"({(time.time() - t0) / (i + 1 - start) * 1e3:.1f} ms/step){tail}")
        if keeper is not None and keeper.after_step(epoch - 1, i, global_step):
            return global_step
    if guard:                                        # every rank, not only the one that logs: the ranks must agree
        import hashlib
        stats, _ = _guard_report(args, optimizer, fused, 0)
        digest, finite = hashlib.sha256(), True
        for p in model.parameters():
            host = p.detach().cpu().numpy()
            digest.update(host.tobytes())
            finite = finite and bool(np.isfinite(host).all())
        print(f"rank {args.rank} epoch {epoch} non-finite guard: skipped {stats['skipped']} parameters "
              f"{'finite' if finite else 'NOT FINITE'} sha256 {digest.hexdigest()[:16]}", flush=True)
    return global_step


def ema_epoch(args, model, ema, raw_result, test, epoch):
    """--ema_decay, after an epoch's evaluation: the same evaluation with the average in the parameters (every line tagged EMA),
    the state's line, with --permutation the paired test of the average against the raw model, with --save_model the average
    as a checkpoint of the model's keys; last, on every rank, the digest of the shadows (the ranks must agree)."""
    with ema.applied():
        ema_result = eval_epoch(args, model, test, tag="EMA")
    n, d = ema.updates(), ema.last_decay()
    log(args, f"ema updates {n} decay {d if d is not None else float('nan'):.6f}")
    if args.permutation:
        from neighborretr_amd.evaluator import compare_evaluations
        cmp = compare_evaluations(ema_result, raw_result, args.permutation, args.permutation_seed, args.bootstrap,
                                  args.bootstrap_seed, args.bootstrap_level, device=args.device)
        _log_comparison(args, cmp, "EMA - model", versus="model")
    if args.rank == 0 and args.save_model:
        torch.save(ema.model_state_dict(model), os.path.join(args.output_dir, f"pytorch_model_ema.bin.{epoch}"))
    print(f"rank {args.rank} epoch {epoch + 1} ema sha256 {ema.sha256()[:16]}", flush=True)
    return ema_result


def _guard_report(args, optimizer, fused, window):
    """--skip_nonfinite 1 -> ({skipped, consecutive, max_consecutive}, the gradient norms of the last `window` steps): from the
    device's guard and record ring (BertAdam; one blocking copy, at a log line only) or from the host's counts (adamw)."""
    if fused:
        stats = optimizer.guard_stats()
        return stats, [float(v) for v in optimizer.records(last=window)["grad_norm"]] if window else []
    hs = args._host_skips
    return hs, hs["norms"][-window:] if window else []


def eval_epoch(args, model, test, tag=""):
    """`tag`: a word every line of this run starts with (EMA: the evaluation of the averaged weights).

    evaluator.py:66-291 for the single-sentence case with the work SHARDED over the ranks (neighborretr_amd.evaluator):
    every rank "extracts" the features of its samples (rank, rank + W, ...: a DistributedSampler's split; feature mode:
    they are the inputs), one packed all-gather + index scatter restores dataset order (evaluator.py:173-189), rank r
    computes rows [r N/W, (r+1) N/W) of the N x N similarity and the rank counts of its slab on the GPU, three small
    collectives complete them."""
    from neighborretr_amd.evaluator import (correction_from_args, gather_eval_features, rank_sample_indices, rerank_ivf_from_args,
                                            rerank_local_scaling_from_args, rerank_mutual_proximity_from_args, rerank_norm_from_args,
                                            rerank_top_from_args, sharded_evaluation, two_stage_evaluation, two_stage_ivf_label, two_stage_label)
    from neighborretr_amd.metrics import RetrievalMetrics
    correction, extras = correction_from_args(args, model)     # every flag checked before any work
    rerank_top = rerank_top_from_args(args)
    rerank_ivf = rerank_ivf_from_args(args)
    rerank_norm = rerank_norm_from_args(args, model)
    rerank_ls = rerank_local_scaling_from_args(args, model)
    rerank_mp = rerank_mutual_proximity_from_args(args, model)
    hubness_k = extras["hubness_k"]
    log = _tagged_log(tag)

    def log_ir(nt, nv, tag=""):
        """The IR line of each direction (MRR, mAP, nDCG@10, R-Prec) and its interval lines."""
        if not extras["ir"]:
            return
        for side, m in (("text->video", nt), ("video->text", nv)):
            prefix = f"{side} {tag}".rstrip() + ": "
            log(args, RetrievalMetrics.format_ir(m["ir"], prefix=prefix))
            for key in ("bootstrap", "bootstrap_vs_raw"):
                if key in m["ir"]:
                    log(args, RetrievalMetrics.format_ir_bootstrap(m["ir"][key], prefix=prefix))

    def log_bootstrap(nt, nv, tag=""):
        """The interval line of each direction after its metrics line, and for a correction the paired line against raw."""
        if not extras["bootstrap"]:
            return
        for side, m in (("text->video", nt), ("video->text", nv)):
            log(args, RetrievalMetrics.format_bootstrap(m["bootstrap"], prefix=f"{side} {tag}".rstrip() + " "))
            if "bootstrap_vs_raw" in m:
                log(args, RetrievalMetrics.format_bootstrap(m["bootstrap_vs_raw"], prefix=f"{side} {tag} - raw "))

    def log_permutation(nt, nv, tag):
        """The paired permutation test of a correction against raw: one line per direction, one for its IR metrics and, with
        --hubness_test, one for its hubness."""
        for side, m in (("text->video", nt), ("video->text", nv)):
            if "permutation_vs_raw" in m:
                log(args, RetrievalMetrics.format_permutation(m["permutation_vs_raw"], prefix=f"{side} {tag} - raw "))
            if "permutation_vs_raw" in m.get("ir", {}):
                log(args, RetrievalMetrics.format_permutation(m["ir"]["permutation_vs_raw"], prefix=f"{side} {tag} - raw "))
            if "permutation_vs_raw" in m.get("hubness", {}):
                log(args, RetrievalMetrics.format_hubness_permutation(m["hubness"]["permutation_vs_raw"], m["hubness"]["k"],
                                                                      prefix=f"{side} {tag} - raw: "))
    model.eval()
    dev = args.device
    mine = rank_sample_indices(test.n, args.world_size, args.rank)     # equal counts on every rank (padded like DistributedSampler)
    if model.feature_mode:
        t, tm, v, vm = (x[mine].to(dev) for x in (test.t, test.tm, test.v, test.vm))
    else:                                                   # evaluator.py:162-171: features cached batch by batch
        parts = [encode(model, test.rows(mine[lo:lo + 32], dev)) for lo in range(0, len(mine), 32)]
        t, tm, v, vm = (torch.cat([p[k] for p in parts], 0) for k in range(4))
    if args.world_size > 1:
        t, v, tm, vm = gather_eval_features(t, v, mine.to(dev), tm, vm, args)
    t2v, v2t = sharded_evaluation(model, t, v, tm.float(), vm.float(), args, correction, **extras)
    log(args, f"text->video R@1 {t2v['R1']:.1f} R@5 {t2v['R5']:.1f} R@10 {t2v['R10']:.1f} MedR {t2v['MR']:.1f} | "
              f"video->text R@1 {v2t['R1']:.1f} R@5 {v2t['R5']:.1f} R@10 {v2t['R10']:.1f} MedR {v2t['MR']:.1f}")
    log_bootstrap(t2v, v2t)
    log_ir(t2v, v2t)
    if hubness_k:
        log(args, RetrievalMetrics.format_hubness(t2v["hubness"], prefix="text->video "))
        log(args, RetrievalMetrics.format_hubness(v2t["hubness"], prefix="video->text "))
    if correction is not None:
        nt, nv, tag = t2v[correction.key], v2t[correction.key], correction.label
        log(args, f"text->video {tag} R@1 {nt['R1']:.1f} R@5 {nt['R5']:.1f} R@10 {nt['R10']:.1f} MedR {nt['MR']:.1f} | "
                  f"video->text {tag} R@1 {nv['R1']:.1f} R@5 {nv['R5']:.1f} R@10 {nv['R10']:.1f} MedR {nv['MR']:.1f}")
        log_bootstrap(nt, nv, tag)
        log_ir(nt, nv, tag)
        log_permutation(nt, nv, tag)
        if hubness_k:
            log(args, RetrievalMetrics.format_hubness(nt["hubness"], prefix=f"text->video {tag} "))
            log(args, RetrievalMetrics.format_hubness(nv["hubness"], prefix=f"video->text {tag} "))
        if "marginal_err" in nt:
            log(args, f"{tag} marginal error {nt['marginal_err']:.3e} / {nv['marginal_err']:.3e}")
    if rerank_top:                                          # two-stage retrieval next to the exhaustive figures, never instead of them
        torch.cuda.synchronize()
        tic = time.time()
        rerank_corr = rerank_mp or rerank_ls or rerank_norm
        norm_kw = dict(rerank_corr, hubness_k=min(hubness_k, rerank_top)) if rerank_corr else {}
        t2v["two_stage"], v2t["two_stage"] = two_stage_evaluation(model, t, v, tm.float(), vm.float(), args, rerank_top, **norm_kw,
                                                                  **(rerank_ivf or {}))
        toc = time.time()
        tag = two_stage_label(rerank_top) if rerank_ivf is None else \
            two_stage_ivf_label(rerank_top, rerank_ivf["n_lists"], rerank_ivf["nprobe"])
        for line in RetrievalMetrics.two_stage_lines(t2v["two_stage"], v2t["two_stage"], tag, ("text->video", "video->text"), " "):
            log(args, line)
        log(args, f"{tag} wall time {toc - tic:.2f}s")
    return t2v, v2t


def compare_with_model(args, result, train, test, with_bank):
    """--compare_model PATH: the test set scored again with the same architecture loaded from PATH, then the "model - compared"
    lines of evaluator.compare_evaluations (result minus that evaluation).  The second model is released before returning."""
    from neighborretr_amd.evaluator import compare_evaluations
    from neighborretr_amd.modeling import NeighborRetr
    other = NeighborRetr(args, precision=args.precision, with_encoders=bool(args.encoders))
    missing, unexpected = other.load_state_dict(torch.load(args.compare_model, map_location="cpu"), strict=False)
    log(args, f"compare_model {args.compare_model}: {len(missing)} missing / {len(unexpected)} unexpected keys")
    other = other.to(args.device)
    if with_bank:
        load_memory_bank(args, other, train)
    compared = eval_epoch(args, other, test)
    del other                                               # the second model (and its memory bank) goes before the summaries
    torch.cuda.empty_cache()
    cmp = compare_evaluations(result, compared, args.permutation, args.permutation_seed, args.bootstrap, args.bootstrap_seed,
                              args.bootstrap_level, device=args.device)

    _log_comparison(args, cmp, "model - compared", versus="compared")
    return cmp


def _log_comparison(args, cmp, what, versus):
    """The lines of evaluator.compare_evaluations' result `cmp` under the prefix `what` ("a - b"; versus: what b is called)."""
    from neighborretr_amd.evaluator import CORRECTION_KEYS
    from neighborretr_amd.metrics import RetrievalMetrics

    def lines(c, prefix):
        log(args, RetrievalMetrics.format_permutation(c["permutation"], prefix=prefix, versus=versus))
        if "bootstrap" in c:
            log(args, RetrievalMetrics.format_bootstrap(c["bootstrap"], prefix=prefix, versus=versus))
        if "ir" in c:
            log(args, RetrievalMetrics.format_permutation(c["ir"]["permutation"], prefix=prefix, versus=versus))
            if "bootstrap" in c["ir"]:
                log(args, RetrievalMetrics.format_ir_bootstrap(c["ir"]["bootstrap"], prefix=prefix, versus=versus))
        if "hubness" in c:
            log(args, RetrievalMetrics.format_hubness_permutation(c["hubness"]["permutation"], c["hubness"]["k"], prefix=prefix,
                                                                  versus=versus))
    for side, c in zip(("text->video", "video->text"), cmp):
        lines(c, f"{what} {side} ")
        for key in CORRECTION_KEYS:
            if key in c:
                lines(c[key], f"{what} {side} [{key}] ")


def main():
    args = get_args()
    args = setup_distributed(args)
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    if not args.synthetic:
        raise SystemExit("datasets / CLIP towers are outside this build (SURVEY.md 2.1): run with --synthetic, "
                         "or import neighborretr_amd.modeling.NeighborRetr into the reference's main.py")
    resume_state = None
    if args.resume is not None:                             # read (and refused) before anything is built
        from neighborretr_amd import checkpoint
        path = os.path.join(args.output_dir, "training_state.pt") if args.resume == "auto" else args.resume
        if args.resume == "auto" and not os.path.exists(path):
            log(args, f"--resume auto: no {path}, a fresh start")
        else:
            try:
                resume_state = checkpoint.load(path, config=checkpoint.config_from_args(args))
            except checkpoint.CheckpointError as err:
                raise SystemExit(f"--resume: {err}")
    from neighborretr_amd.modeling import NeighborRetr
    model = NeighborRetr(args, precision=args.precision, with_encoders=bool(args.encoders))
    if args.init_model:
        sd = torch.load(args.init_model, map_location="cpu")
        missing, unexpected = model.load_state_dict(sd, strict=False)          # main.py:60-67
        log(args, f"init_model: {len(missing)} missing / {len(unexpected)} unexpected keys")
    model = model.to(args.device)
    ddp = model
    # (--hip_graph 1 replays the whole data-parallel step, gradient average included, from graphs: GraphedStep; a DDP wrapper
    # would keep AccumulateGrad nodes of the default stream alive, which a capture must not be synchronised with)
    if args.world_size > 1 and not args.hip_graph:
        ddp = torch.nn.parallel.DistributedDataParallel(model, device_ids=[args.device_index],
                                                        find_unused_parameters=True)   # optimizer.py:79-84
    Data = SyntheticClips if args.encoders else SyntheticFeatures
    train = Data(args, args.synthetic_train, "train", args.seed)
    test = Data(args, args.synthetic_test, "test", args.seed + 1)
    ema = None
    if args.ema_decay:
        from neighborretr_amd.optim import WeightEma
        ema = WeightEma(model.named_parameters(), decay=args.ema_decay, warmup=bool(args.ema_warmup))
    if args.optimizer == "bertadam":
        from neighborretr_amd.optim import prep_optimizer
        # (wrap=False: the model is wrapped above, or not at all under --hip_graph 1)
        optimizer = prep_optimizer(args, model, len(train) * args.epochs, args.device_index, global_max_norm=1.0,
                                   clamp_logit_scale=True, wrap=False, skip_nonfinite=bool(args.skip_nonfinite), ema=ema)[0]
    else:
        optimizer = torch.optim.AdamW(model.parameters(), lr=args.lr, weight_decay=args.weight_decay)
    os.makedirs(args.output_dir, exist_ok=True)
    global_step = 0
    if args.do_train:
        keeper, first_epoch, first_step = None, 0, 0
        if args.save_state_every or args.max_steps or args.resume is not None:
            keeper = StateKeeper(args, model, optimizer, ema)
        if resume_state is not None:
            pos = resume_training(args, resume_state, keeper)
            first_epoch, first_step, global_step = pos["epoch"], pos["next_step"], pos["global_step"]
            del resume_state
        for epoch in range(first_epoch, args.epochs):
            start = first_step if epoch == first_epoch else 0
            if start == 0:                                  # (a run resumed inside an epoch goes on with the restored bank)
                load_memory_bank(args, model, train)
            global_step = train_epoch(args, model, ddp, train, optimizer, epoch + 1, global_step,
                                      ema=ema if args.optimizer != "bertadam" else None, start=start, keeper=keeper)
            if keeper is not None and keeper.stopped:
                log(args, f"--max_steps {args.max_steps}: stopped after global step {global_step}")
                break
            raw_result = eval_epoch(args, model, test)
            if args.rank == 0 and args.save_model:
                torch.save(model.state_dict(), os.path.join(args.output_dir, f"pytorch_model.bin.{epoch}"))
            if ema is not None:
                ema_epoch(args, model, ema, raw_result, test, epoch)
            if keeper is not None:
                keeper.end_of_epoch(epoch, global_step)
            clear_memory_bank(model)
    elif args.do_eval:
        with_bank = args.test_norm in ("qbnorm", "qbsinkhorn") or (args.local_scaling != "none" and args.local_scaling_bank) \
            or (args.mutual_proximity != "none" and args.mutual_proximity_bank) or args.rerank_norm != "none" \
            or args.rerank_local_scaling != "none" or args.rerank_mutual_proximity != "none"
        if with_bank:                                      # the querybank: the memory bank of the training set
            load_memory_bank(args, model, train)
        result = eval_epoch(args, model, test)
        if with_bank:
            clear_memory_bank(model)
        if args.compare_model:
            compare_with_model(args, result, train, test, with_bank)
    if args.world_size > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
