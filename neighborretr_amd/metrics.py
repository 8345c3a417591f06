"""Retrieval metrics with the rank counting done on the GPU.

Same interface as the reference's NeighborRetr/utils/metrics.py:14-79 (`RetrievalMetrics`,
`compute_metrics` returning R1/R5/R10/R50/MR/MedianR/MeanR/cols).  The reference sorts every row
on the host (np.sort) and looks up where the diagonal landed; the rank of the diagonal is just
#{j : S[i,j] > S[i,i]}, and its exact-equality tie rule (`where(sx - d == 0)`) yields one hit per
entry EQUAL to the diagonal, at consecutive ranks.  nr_diag_ranks counts both on the device in
one pass over S; only 2N integers come back to the host.
"""
import numpy as np
import torch

from . import ops


class RetrievalMetrics:
    def __init__(self, logger=None):
        self.best_mean_r1 = 0.00001
        self.best_t2v_r1 = 0.00001
        self.best_v2t_r1 = 0.00001
        self.best_t2v_metrics = None
        self.best_v2t_metrics = None
        self.logger = logger

    @staticmethod
    def diagonal_ranks(similarity_matrix):
        """`ind` of metrics.py:58-66: for row i the ranks greater[i] .. greater[i]+equal[i]-1."""
        S = similarity_matrix
        if not torch.is_tensor(S):
            S = torch.from_numpy(np.ascontiguousarray(S, dtype=np.float32))
        if not S.is_cuda:
            S = S.cuda()
        greater, equal = ops.diag_ranks(S)
        return RetrievalMetrics.ranks_from_counts(greater.cpu().numpy(), equal.cpu().numpy())

    @staticmethod
    def ranks_from_counts(greater, equal):
        """`ind` from the per-row counts #{j: S[i,j] > S[i,i]} and #{j: S[i,j] == S[i,i]} (the latter includes the diagonal):
        row i contributes the consecutive ranks greater[i] .. greater[i] + equal[i] - 1, rows in order."""
        greater, equal = np.asarray(greater, dtype=np.int64), np.asarray(equal, dtype=np.int64)
        return np.repeat(greater, equal) + (np.arange(int(equal.sum())) - np.repeat(np.cumsum(equal) - equal, equal))

    @staticmethod
    def compute_metrics(similarity_matrix):
        return RetrievalMetrics.metrics_from_ranks(RetrievalMetrics.diagonal_ranks(similarity_matrix))

    @staticmethod
    def metrics_from_ranks(ind):
        n = len(ind)
        m = {
            "R1": float(np.sum(ind == 0)) * 100 / n,
            "R5": float(np.sum(ind < 5)) * 100 / n,
            "R10": float(np.sum(ind < 10)) * 100 / n,
            "R50": float(np.sum(ind < 50)) * 100 / n,
            "MR": float(np.median(ind)) + 1,
        }
        m["MedianR"] = m["MR"]
        m["MeanR"] = float(np.mean(ind)) + 1
        m["cols"] = [int(i) for i in ind]
        return m

    @staticmethod
    def tensor_text_to_video_metrics(sim_tensor, top_k=(1, 5, 10, 50)):
        """Multi-sentence text->video metrics with the reference's interface (utils/metrics.py:82-126): `sim_tensor[i, s, j]` =
        score of sentence s of video i against video j, -inf / NaN where video i has fewer sentences.  The rank of every valid
        sentence's own video is COUNTED -- scores above its own (NaN scores sort first) plus equal scores at lower video
        indices, i.e. a stable descending order, the rule of nr_group_slab_ranks -- instead of sorted out of the padded tensor;
        the product's evaluator never builds that tensor (neighborretr_amd.evaluator: row slabs + nr_group_slab_ranks)."""
        sim = torch.as_tensor(sim_tensor)
        n_video = sim.shape[0]
        video = torch.arange(n_video, device=sim.device)
        own = sim[video, :, video]                                        # [video, sentence]: the sentence against its own video
        ahead = (sim > own[:, :, None]) | torch.isnan(sim)
        ahead |= (sim == own[:, :, None]) & (video[None, None, :] < video[:, None, None])
        ranks = ahead.sum(-1)[torch.isfinite(own)]
        return RetrievalMetrics.multi_sentence_metrics_from_ranks(ranks.cpu(), top_k)

    @staticmethod
    def multi_sentence_metrics_from_ranks(ranks, top_k=(1, 5, 10, 50)):
        """The result dictionary of metrics.py:113-126 from the 0-based rank of every valid sentence's own video."""
        valid = torch.as_tensor(ranks).to(torch.int64).cpu()
        res = {f"R{k}": float(torch.sum(valid < k) * 100 / len(valid)) for k in top_k}
        res["MedianR"] = float(torch.median(valid + 1))
        res["MeanR"] = float(np.mean(valid.numpy() + 1))
        res["Std_Rank"] = float(np.std(valid.numpy() + 1))
        res["MR"] = res["MedianR"]
        return res

    @staticmethod
    def tensor_video_to_text_sim(sim_tensor):
        """[n_video, max_sentences, n_video] -> the [n_video, n_video] video->text matrix: entry (j, i) = the best score any
        sentence of caption group i reaches against video j (utils/metrics.py:128-148); NaN padding never wins, and the
        caller's tensor is left as it was."""
        sim = torch.as_tensor(sim_tensor)
        return torch.nan_to_num(sim, nan=float("-inf"), posinf=float("inf"), neginf=float("-inf")).amax(dim=1).T

    @staticmethod
    def hubness_from_occurrences(occ, good, k, n_queries):
        """Hubness summary of one direction from its k-occurrence counts (DESIGN.md "Top-k lists and hubness"): occ[j] = N_k
        of gallery item j (queries whose top-k list holds j), good[j] = GN_k (those for which j is a ground truth).  Hubs are
        the items with N_k > 2 mu; percentages follow the R@K convention (count * 100 / n)."""
        occ = np.asarray(occ, dtype=np.int64).reshape(-1)
        good = np.asarray(good, dtype=np.int64).reshape(-1)
        if occ.shape != good.shape or occ.size == 0:
            raise ValueError("occ and good must be non-empty and of one length")
        n = occ.size
        total = int(occ.sum())
        mu = total / n
        dev = occ.astype(np.float64) - mu
        std = float(np.sqrt(np.mean(dev ** 2)))
        skew = float(np.mean(dev ** 3) / std ** 3) if std > 0 else 0.0
        hubs = occ > 2 * mu
        bad = occ - good
        return {
            "k": int(k),
            "n_queries": int(n_queries),
            "n_gallery": int(n),
            "mu": float(mu),
            "skewness": skew,
            "anti_hub_pct": float(np.sum(occ == 0)) * 100 / n,
            "hub_pct": float(np.sum(hubs)) * 100 / n,
            "hub_occurrence_pct": float(np.sum(occ[hubs])) * 100 / total if total else 0.0,
            "bad_hub_pct": float(np.sum(hubs & (bad > good))) * 100 / n,
            "good_occurrence_pct": float(np.sum(good)) * 100 / total if total else 0.0,
            "max_occurrence": int(occ.max()),
            "occurrence": occ,
            "good_occurrence": good,
        }

    @staticmethod
    def format_two_stage(m, prefix=""):
        """One line of a two-stage direction (evaluator.two_stage_evaluation): R@K where K <= C, the candidate recall and, when
        every query was found, MedR."""
        recalls = " ".join(f"R@{K} {m[f'R{K}']:.1f}" for K in (1, 5, 10, 50) if m.get(f"R{K}") is not None)
        line = f"{prefix}{recalls} - candidate recall {m['cand_recall']:.1f}%"
        line += f" - MedR {m['MR']:.1f}" if "MR" in m else ""
        return line + (f" - normalised {m['gated']:.1f}% of the queries" if "gated" in m else "")

    @staticmethod
    def two_stage_lines(t2v, v2t, tag, sides=("Text-to-Video", "Video-to-Text"), sep=": "):
        """The log lines of evaluator.two_stage_evaluation: one per direction tagged `tag`; with a query-bank normalisation one
        more per direction tagged with its label ("[two-stage C=64 QB-Norm b=20 k=1]", with the gated share), with local scaling
        one more tagged with its own ("[two-stage C=64 QB-CSLS k=10]"), with mutual proximity likewise ("[two-stage C=64 QB-MP-emp]");
        with hubness, the line of each dictionary's top-K lists after it."""
        lines = []
        for pick in (lambda m: m, lambda m: m.get("normalised"), lambda m: m.get("local_scaled"),
                     lambda m: m.get("mutual_proximity")):
            for side, raw in zip(sides, (t2v, v2t)):
                m = pick(raw)
                if m is None:
                    continue
                label = m.get("label", tag)
                lines.append(RetrievalMetrics.format_two_stage(m, prefix=f"{side} {label}{sep}"))
                if "ivf_overlap" in m:           # the inverted-file prefilter: one more line per direction
                    lines.append(f"{side} {label}{sep}pool {m['pool_mean'] * 100:.1f}% of the gallery - kept "
                                 f"{m['ivf_overlap'] * 100:.1f}% of the exact prefilter's candidates")
                if "hubness" in m:
                    lines.append(RetrievalMetrics.format_hubness(m["hubness"], prefix=f"{side} {label} "))
        return lines

    @staticmethod
    def format_hubness(hub, prefix=""):
        return (f"{prefix}Hubness@{hub['k']}: skew {hub['skewness']:.2f} - hubs {hub['hub_pct']:.1f}% - "
               f"hub occurrence {hub['hub_occurrence_pct']:.1f}% - bad hubs {hub['bad_hub_pct']:.1f}% - "
               f"anti-hubs {hub['anti_hub_pct']:.1f}% - good occurrence {hub['good_occurrence_pct']:.1f}% - "
               f"max N_k {hub['max_occurrence']}")

    def log_hubness(self, hub, prefix=""):
        """One line per direction, in the style of print_metrics (silent without a logger)."""
        if self.logger is not None:
            self.logger.info(self.format_hubness(hub, prefix))

    # ---- bootstrap confidence intervals (DESIGN.md "Bootstrap confidence intervals") ----------------------------------------------
    BOOTSTRAP_LOGGED = ("R1", "R5", "R10", "MedianR", "MeanR")            # the metrics of the log line, where present

    @staticmethod
    def _bootstrap_values(stats, cuts, median):
        """({metric: fp64 array over the rows of stats}, n) from rows (n, sum, med_lo, med_hi, hits...); rows with n = 0 give NaN."""
        if median not in ("mid", "low"):
            raise ValueError(f"median must be 'mid' (np.median) or 'low' (torch.median), got {median!r}")
        if torch.is_tensor(stats):
            stats = stats.cpu().numpy()
        stats = np.asarray(stats, dtype=np.int64)
        cuts = [int(c) for c in cuts]
        if stats.ndim != 2 or stats.shape[1] != 4 + len(cuts):
            raise ValueError(f"stats must be [n_boot, {4 + len(cuts)}] for {len(cuts)} cut-offs, got {stats.shape}")
        n = stats[:, 0].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            vals = {f"R{c}": 100 * stats[:, 4 + k].astype(np.float64) / n for k, c in enumerate(cuts)}
            med_hi = stats[:, 3] if median == "mid" else stats[:, 2]
            vals["MedianR"] = np.where(n > 0, (stats[:, 2] + med_hi).astype(np.float64) / 2 + 1, np.nan)
            vals["MeanR"] = stats[:, 1].astype(np.float64) / n + 1
        return vals, stats[:, 0]

    @staticmethod
    def _entry_stats(entries, cuts):
        """The row (n, sum, med_lo, med_hi, hits...) of the un-resampled entries."""
        r = np.sort(np.asarray(entries, dtype=np.int64).reshape(-1))
        n = len(r)
        med = [int(r[(n - 1) // 2]), int(r[n // 2])] if n else [-1, -1]
        return np.asarray([[n, int(r.sum())] + med + [int((r < int(c)).sum()) for c in cuts]], dtype=np.int64)

    @staticmethod
    def _interval(x, point, level):
        """point, standard error (population sd) and percentile interval of the resampled values x."""
        if len(x) == 0:
            return {"point": point, "se": float("nan"), "lo": float("nan"), "hi": float("nan")}
        lo, hi = np.percentile(x, [100 * (1 - level) / 2, 100 * (1 + level) / 2])
        return {"point": point, "se": float(np.std(x)), "lo": float(lo), "hi": float(hi)}

    @staticmethod
    def _check_level(level):
        level = float(level)
        if not 0.0 < level < 1.0:
            raise ValueError(f"bootstrap level must lie in (0, 1), got {level!r}")
        return level

    @staticmethod
    def bootstrap_summary(stats, cuts, entries, level=0.95, median="mid"):
        """Percentile bootstrap of one ranking: stats [n_boot, 4 + K] int64 (ops.bootstrap_rank_stats[:, v]), entries = its
        un-resampled ranks.  Per resample with n > 0: R{c} = 100 hits / n, MeanR = sum / n + 1, MedianR = (med_lo + med_hi) / 2 + 1
        (median "mid": np.median) or med_lo + 1 ("low": torch.median).  -> {"n_boot", "n_empty" (resamples with n = 0, dropped),
        "level", "median", and per metric {"point" (the formula on `entries`), "se" (population sd over the resamples), "lo", "hi"
        (np.percentile at 100 (1 -+ level) / 2)}}."""
        level = RetrievalMetrics._check_level(level)
        vals, n = RetrievalMetrics._bootstrap_values(stats, cuts, median)
        point, _ = RetrievalMetrics._bootstrap_values(RetrievalMetrics._entry_stats(entries, cuts), cuts, median)
        keep = n > 0
        out = {"n_boot": int(len(n)), "n_empty": int(np.sum(~keep)), "level": level, "median": median}
        for name, x in vals.items():
            out[name] = RetrievalMetrics._interval(x[keep], float(point[name][0]), level)
        return out

    @staticmethod
    def paired_bootstrap_summary(stats, stats_raw, cuts, entries, entries_raw, level=0.95, median="mid"):
        """Paired bootstrap of "corrected minus raw": stats / stats_raw [n_boot, 4 + K] of the two rankings of ONE V = 2 call (the
        same draws).  The fields of bootstrap_summary for the per-resample differences, and per metric "frac_le0" / "frac_ge0": the
        share of resamples whose difference is <= 0 / >= 0.  A resample empty in either ranking is dropped (n_empty)."""
        level = RetrievalMetrics._check_level(level)
        a, na = RetrievalMetrics._bootstrap_values(stats, cuts, median)
        b, nb = RetrievalMetrics._bootstrap_values(stats_raw, cuts, median)
        if len(na) != len(nb):
            raise ValueError("paired bootstrap: the two rankings must come from one call (the same resamples)")
        pa, _ = RetrievalMetrics._bootstrap_values(RetrievalMetrics._entry_stats(entries, cuts), cuts, median)
        pb, _ = RetrievalMetrics._bootstrap_values(RetrievalMetrics._entry_stats(entries_raw, cuts), cuts, median)
        keep = (na > 0) & (nb > 0)
        out = {"n_boot": int(len(na)), "n_empty": int(np.sum(~keep)), "level": level, "median": median}
        for name in a:
            d = a[name][keep] - b[name][keep]
            out[name] = RetrievalMetrics._interval(d, float(pa[name][0] - pb[name][0]), level)
            out[name]["frac_le0"] = float(np.mean(d <= 0)) if len(d) else float("nan")
            out[name]["frac_ge0"] = float(np.mean(d >= 0)) if len(d) else float("nan")
        return out

    @staticmethod
    def format_bootstrap(summary, prefix="", versus="raw"):
        """One line: every logged metric with its interval; a paired summary prints signed differences and frac_le0 (versus: what
        the pair's second ranking is called)."""
        paired = any(isinstance(v, dict) and "frac_le0" in v for v in summary.values())
        label = {"R1": "R@1", "R5": "R@5", "R10": "R@10", "MedianR": "Median R", "MeanR": "Mean R"}
        parts = []
        for name in RetrievalMetrics.BOOTSTRAP_LOGGED:
            if name not in summary:
                continue
            m = summary[name]
            if paired:
                parts.append(f"{label[name]}: {m['point']:+.1f} [{m['lo']:+.1f}, {m['hi']:+.1f}] frac<=0 {m['frac_le0']:.3f}")
            else:
                parts.append(f"{label[name]}: {m['point']:.1f} [{m['lo']:.1f}, {m['hi']:.1f}]")
        kind = f"paired bootstrap vs {versus}" if paired else "bootstrap"
        tail = f" ({100 * summary['level']:g}% {kind}, {summary['n_boot']} resamples"
        tail += f", {summary['n_empty']} empty)" if summary["n_empty"] else ")"
        return prefix + " - ".join(parts) + tail

    def log_bootstrap(self, summary, prefix=""):
        """One line per summary, in the style of print_metrics (silent without a logger)."""
        if self.logger is not None:
            self.logger.info(self.format_bootstrap(summary, prefix))

    # ---- rank-aware IR metrics: MRR, mAP, nDCG@10, R-precision (DESIGN.md "Rank-aware IR metrics") --------------------------------
    IR_METRICS = ("MRR", "mAP", "nDCG10", "RPrec")
    IR_LABELS = {"MRR": "MRR", "mAP": "mAP", "nDCG10": "nDCG@10", "RPrec": "R-Prec"}
    IR_FIXED_ONE = 1 << 32                                                # the fixed-point image of 1.0 in the bootstrap's columns

    @staticmethod
    def _ir_group_ends(group_end, n):
        ends = np.asarray(group_end, dtype=np.int64).reshape(-1)
        if len(ends) == 0 or ends[0] < 1 or (np.diff(ends) < 1).any() or ends[-1] != n:
            raise ValueError(f"group_end must be positive, increasing and end at the {n} ranks")
        return ends

    @staticmethod
    def _ir_queries(ranks, group_end=None):
        """(values fp64 [n_slots, 4]: RR, AP, nDCG10, RPrec in [0, 1] of every query slot, zeros where the slot has no ranked pair;
        valid bool [n_slots]).  group_end None: every entry of `ranks` is a query with one relevant item (m = 1); otherwise slot g
        is the query of the entries [group_end[g-1], group_end[g]).  ranks < 0 are unranked pairs."""
        ranks = np.asarray(ranks, dtype=np.int64).reshape(-1)
        if group_end is None:
            valid = ranks >= 0
            r = np.where(valid, ranks, 0).astype(np.float64)
            rr = np.where(valid, 1.0 / (r + 1.0), 0.0)
            ndcg = np.where(valid & (ranks < 10), 1.0 / np.log2(r + 2.0), 0.0)          # IDCG of m = 1 is 1 / log2(2) = 1
            return np.stack([rr, rr, ndcg, (valid & (ranks == 0)).astype(np.float64)], axis=1), valid
        ends = RetrievalMetrics._ir_group_ends(group_end, len(ranks))
        values = np.zeros((len(ends), 4), dtype=np.float64)
        valid = np.zeros((len(ends),), dtype=bool)
        begin = 0
        for g, end in enumerate(ends):
            seg = ranks[begin:end]
            begin = end
            r = np.sort(seg[seg >= 0]).astype(np.float64)
            m = len(r)
            if m == 0:
                continue
            k = np.arange(1, m + 1, dtype=np.float64)
            dcg = float(np.sum(1.0 / np.log2(r[r < 10] + 2.0)))
            idcg = float(np.sum(1.0 / np.log2(k[:10] + 1.0)))
            values[g] = (1.0 / (r[0] + 1.0), float(np.sum(k / (r + 1.0))) / m, dcg / idcg, float(np.sum(r < m)) / m)
            valid[g] = True
        return values, valid

    @staticmethod
    def ir_from_ranks(ranks, group_end=None):
        """MRR, mAP, nDCG@10 and R-precision (means over the queries x 100, like R@K) from the 0-based ranks of the relevant
        (sentence, video) pairs, < 0 where a pair is unranked.  group_end None: every pair is a query of its own (text->video, and
        both directions of a single-sentence set); otherwise query g (a video) owns the pairs [group_end[g-1], group_end[g]) and
        its ranks are distinct (video->text over all sentences).  Per query with sorted ranked ranks r_1 < ... < r_m:
        RR = 1 / (r_1 + 1), AP = mean_k k / (r_k + 1), nDCG10 = sum_{r_k < 10} 1 / log2(r_k + 2) over sum_{k <= min(m, 10)}
        1 / log2(k + 1), RPrec = #{r_k < m} / m.  A query without a ranked pair is dropped.  -> {"MRR", "mAP", "nDCG10", "RPrec",
        "n_queries", "n_unranked" (pairs), "ranks" (int64, -1 for unranked pairs)}."""
        ranks = np.asarray(ranks.cpu() if torch.is_tensor(ranks) else ranks, dtype=np.int64).reshape(-1)
        values, valid = RetrievalMetrics._ir_queries(ranks, group_end)
        n = int(valid.sum())
        out = {name: float(values[valid, i].mean()) * 100 if n else float("nan") for i, name in enumerate(RetrievalMetrics.IR_METRICS)}
        out.update(n_queries=n, n_unranked=int(np.sum(ranks < 0)), ranks=np.where(ranks < 0, -1, ranks))
        return out

    @staticmethod
    def ir_unit_columns(ranks, group_end=None, unit_end=None):
        """int64 [U, 5], the bootstrap's columns of one ranking: per resampling unit its query count and the sums over its queries
        of int(rint(x 2^32)) for x = RR, AP, nDCG10, RPrec.  Queries as in ir_from_ranks; the unit is the query, or with unit_end
        (group_end None: multi-sentence text->video) unit u owns the queries [unit_end[u-1], unit_end[u]).  A unit without a
        ranked pair is a row of zeros."""
        ranks = np.asarray(ranks.cpu() if torch.is_tensor(ranks) else ranks, dtype=np.int64).reshape(-1)
        values, valid = RetrievalMetrics._ir_queries(ranks, group_end)
        cols = np.concatenate([valid[:, None].astype(np.int64), np.rint(values * RetrievalMetrics.IR_FIXED_ONE).astype(np.int64)], axis=1)
        if unit_end is None:
            return cols
        if group_end is not None:
            raise ValueError("unit_end groups single-pair queries: it cannot be combined with group_end")
        ends = RetrievalMetrics._ir_group_ends(unit_end, len(ranks))
        run = np.concatenate([np.zeros((1, cols.shape[1]), dtype=np.int64), np.cumsum(cols, axis=0)])
        return run[ends] - run[np.concatenate(([0], ends[:-1]))]

    @staticmethod
    def _ir_values(sums):
        """({metric: 100 sum_fixed / (2^32 count), NaN where count = 0}, count) of rows (count, RR, AP, nDCG10, RPrec sums)."""
        sums = np.asarray(sums.cpu() if torch.is_tensor(sums) else sums, dtype=np.int64)
        if sums.ndim != 2 or sums.shape[1] != 1 + len(RetrievalMetrics.IR_METRICS):
            raise ValueError(f"sums must be [n, {1 + len(RetrievalMetrics.IR_METRICS)}], got {sums.shape}")
        count = sums[:, 0]
        with np.errstate(divide="ignore", invalid="ignore"):
            vals = {name: np.where(count > 0, 100 * sums[:, 1 + i].astype(np.float64)
                                   / (float(RetrievalMetrics.IR_FIXED_ONE) * count.astype(np.float64)), np.nan)
                    for i, name in enumerate(RetrievalMetrics.IR_METRICS)}
        return vals, count

    @staticmethod
    def ir_bootstrap_summary(sums, columns, level=0.95):
        """Percentile bootstrap of one ranking's IR metrics: sums [n_boot, 5] int64 (ops.bootstrap_unit_sums of `columns`), columns
        = ir_unit_columns.  Per resample with count > 0: metric = 100 sum_fixed / (2^32 count).  -> {"n_boot", "n_empty" (resamples
        with count 0, dropped), "level", and per metric "point" (the formula on the columns' totals), "se", "lo", "hi" as in
        bootstrap_summary}."""
        level = RetrievalMetrics._check_level(level)
        vals, count = RetrievalMetrics._ir_values(sums)
        point, _ = RetrievalMetrics._ir_values(np.asarray(columns, dtype=np.int64).sum(axis=0, keepdims=True))
        keep = count > 0
        out = {"n_boot": int(len(count)), "n_empty": int(np.sum(~keep)), "level": level}
        for name, x in vals.items():
            out[name] = RetrievalMetrics._interval(x[keep], float(point[name][0]), level)
        return out

    @staticmethod
    def ir_paired_bootstrap_summary(sums, columns, columns_raw, level=0.95):
        """Paired bootstrap of "corrected minus raw": sums [n_boot, 10] int64 of ONE ops.bootstrap_unit_sums call on the corrected
        ranking's columns next to the raw ranking's (the same draws).  The fields of ir_bootstrap_summary for the per-resample
        differences, and per metric "frac_le0" / "frac_ge0".  A resample with count 0 in either ranking is dropped (n_empty)."""
        level = RetrievalMetrics._check_level(level)
        sums = np.asarray(sums.cpu() if torch.is_tensor(sums) else sums, dtype=np.int64)
        q = 1 + len(RetrievalMetrics.IR_METRICS)
        if sums.ndim != 2 or sums.shape[1] != 2 * q:
            raise ValueError(f"paired sums must be [n_boot, {2 * q}] (corrected, then raw), got {sums.shape}")
        a, na = RetrievalMetrics._ir_values(sums[:, :q])
        b, nb = RetrievalMetrics._ir_values(sums[:, q:])
        pa, _ = RetrievalMetrics._ir_values(np.asarray(columns, dtype=np.int64).sum(axis=0, keepdims=True))
        pb, _ = RetrievalMetrics._ir_values(np.asarray(columns_raw, dtype=np.int64).sum(axis=0, keepdims=True))
        keep = (na > 0) & (nb > 0)
        out = {"n_boot": int(len(na)), "n_empty": int(np.sum(~keep)), "level": level}
        for name in a:
            d = a[name][keep] - b[name][keep]
            out[name] = RetrievalMetrics._interval(d, float(pa[name][0] - pb[name][0]), level)
            out[name]["frac_le0"] = float(np.mean(d <= 0)) if len(d) else float("nan")
            out[name]["frac_ge0"] = float(np.mean(d >= 0)) if len(d) else float("nan")
        return out

    @staticmethod
    def format_ir(ir, prefix=""):
        return prefix + " - ".join(f"{RetrievalMetrics.IR_LABELS[name]} {ir[name]:.1f}" for name in RetrievalMetrics.IR_METRICS)

    @staticmethod
    def format_ir_bootstrap(summary, prefix="", versus="raw"):
        """One line: every IR metric with its interval; a paired summary prints signed differences and frac_le0 (versus: what the
        pair's second ranking is called)."""
        paired = any(isinstance(v, dict) and "frac_le0" in v for v in summary.values())
        parts = []
        for name in RetrievalMetrics.IR_METRICS:
            m = summary[name]
            if paired:
                parts.append(f"{RetrievalMetrics.IR_LABELS[name]} {m['point']:+.1f} [{m['lo']:+.1f}, {m['hi']:+.1f}] "
                             f"frac<=0 {m['frac_le0']:.3f}")
            else:
                parts.append(f"{RetrievalMetrics.IR_LABELS[name]} {m['point']:.1f} [{m['lo']:.1f}, {m['hi']:.1f}]")
        kind = f"paired bootstrap vs {versus}" if paired else "bootstrap"
        tail = f" ({100 * summary['level']:g}% {kind}, {summary['n_boot']} resamples"
        tail += f", {summary['n_empty']} empty)" if summary["n_empty"] else ")"
        return prefix + " - ".join(parts) + tail

    def log_ir(self, ir, prefix=""):
        """The IR line of one direction and, when present, its interval lines (silent without a logger)."""
        if self.logger is None:
            return
        self.logger.info(self.format_ir(ir, prefix))
        for key in ("bootstrap", "bootstrap_vs_raw"):
            if key in ir:
                self.logger.info(self.format_ir_bootstrap(ir[key], prefix))

    # ---- paired permutation tests (DESIGN.md "Paired permutation tests") ----------------------------------------------------------------
    @staticmethod
    def _permutation_p_values(out, ratios_x, ratios_y, ratios_a, ratios_b, keep):
        """Fills out[metric] = {"diff", "p_two", "p_ge", "p_le"} from {metric: (numerator, denominator)} of the sides X, Y (object
        arrays of Python ints over the kept permutations, denominators > 0) and of the un-permuted A, B (Python ints, or None when
        one of them is empty: every figure is NaN).  d_p = x - y against d_0 = a - b on cross-multiplied integers: never in fp64."""
        kept = int(np.sum(keep))
        for name in ratios_x:
            if ratios_a is None:
                out[name] = {"diff": float("nan"), "p_two": float("nan"), "p_ge": float("nan"), "p_le": float("nan")}
                continue
            (xn, xd), (yn, yd), (an, ad), (bn, bd) = ratios_x[name], ratios_y[name], ratios_a[name], ratios_b[name]
            n0, m0 = an * bd - bn * ad, ad * bd                                  # d_0 = n0 / m0
            left = (xn * yd - yn * xd) * m0                                      # d_p >= d_0  <=>  left >= right (all denominators > 0)
            right = n0 * (xd * yd)
            two, ge, le = (int(np.sum(c)) for c in (abs(left) >= abs(right), left >= right, left <= right)) if kept else (0, 0, 0)
            out[name] = {"diff": n0 / m0, "p_two": (1 + two) / (1 + kept), "p_ge": (1 + ge) / (1 + kept), "p_le": (1 + le) / (1 + kept)}
        return out

    @staticmethod
    def _rank_ratios(stats, cuts, median):
        """{metric: (numerator, denominator)} of rows (n, sum, med_lo, med_hi, hits...) as Python ints (object arrays): R{c} =
        100 hits / n, MeanR = sum / n, MedianR = (med_lo + med_hi) / 2 or 2 med_lo / 2; the "+ 1" of the rank metrics cancels."""
        stats = np.asarray(stats, dtype=np.int64).astype(object)
        n = stats[..., 0]
        out = {f"R{int(c)}": (100 * stats[..., 4 + k], n) for k, c in enumerate(cuts)}
        out["MedianR"] = (stats[..., 2] + (stats[..., 3] if median == "mid" else stats[..., 2]), 2 + 0 * n)
        out["MeanR"] = (stats[..., 1], n)
        return out

    @staticmethod
    def permutation_summary(stats, cuts, entries, entries_other, median="mid", seed=0):
        """Paired permutation (randomisation) test of "ranking A minus ranking B": stats [n_perm, 2, 4 + K] int64
        (ops.permtest_rank_stats: the sides X, Y of every relabelling), entries / entries_other = the un-permuted ranks of A / B.
        Per side the formulas of bootstrap_summary; d_p = m(X_p) - m(Y_p), d_0 = m(A) - m(B).  Permutations with an empty side are
        dropped (n_empty); kept = the rest.  -> {"n_perm", "n_empty", "kept", "seed", "median", and per metric "diff" (d_0),
        "p_two" = (1 + #{|d_p| >= |d_0|}) / (1 + kept), "p_ge" (d_p >= d_0), "p_le" (d_p <= d_0)}.  The comparisons are made on
        cross-multiplied Python integers: the statistic is discrete, ties with d_0 are common and fp64 would break them."""
        if median not in ("mid", "low"):
            raise ValueError(f"median must be 'mid' (np.median) or 'low' (torch.median), got {median!r}")
        stats = np.asarray(stats.cpu() if torch.is_tensor(stats) else stats, dtype=np.int64)
        cuts = [int(c) for c in cuts]
        if stats.ndim != 3 or stats.shape[1:] != (2, 4 + len(cuts)):
            raise ValueError(f"stats must be [n_perm, 2, {4 + len(cuts)}] for {len(cuts)} cut-offs, got {stats.shape}")
        keep = (stats[:, 0, 0] > 0) & (stats[:, 1, 0] > 0)
        out = {"n_perm": int(len(stats)), "n_empty": int(np.sum(~keep)), "kept": int(np.sum(keep)), "seed": int(seed), "median": median}
        x = RetrievalMetrics._rank_ratios(stats[keep, 0], cuts, median)
        y = RetrievalMetrics._rank_ratios(stats[keep, 1], cuts, median)
        a, b = RetrievalMetrics._entry_stats(entries, cuts)[0], RetrievalMetrics._entry_stats(entries_other, cuts)[0]
        if a[0] == 0 or b[0] == 0:
            return RetrievalMetrics._permutation_p_values(out, x, y, None, None, keep)
        return RetrievalMetrics._permutation_p_values(out, x, y, RetrievalMetrics._rank_ratios(a, cuts, median),
                                                      RetrievalMetrics._rank_ratios(b, cuts, median), keep)

    @staticmethod
    def _ir_ratios(sums):
        """{metric: (100 sum_fixed, 2^32 count)} of rows (count, RR, AP, nDCG10, RPrec sums) as Python ints (object arrays)."""
        sums = np.asarray(sums).astype(object)
        return {name: (100 * sums[..., 1 + i], RetrievalMetrics.IR_FIXED_ONE * sums[..., 0])
                for i, name in enumerate(RetrievalMetrics.IR_METRICS)}

    @staticmethod
    def ir_permutation_summary(sums, columns, columns_other, seed=0):
        """Paired permutation test of the IR metrics of "ranking A minus ranking B": sums [n_perm, 5] int64 (ops.permtest_unit_sums of
        the two rankings' ir_unit_columns: side X), columns / columns_other = those columns [U, 5] of A / B; side Y is the two totals
        minus X, in exact integers.  Per side the formula of ir_bootstrap_summary (100 sum_fixed / (2^32 count)); the fields of
        permutation_summary without "median", the comparisons on the fixed-point sums over the counts."""
        sums = np.asarray(sums.cpu() if torch.is_tensor(sums) else sums, dtype=np.int64)
        q = 1 + len(RetrievalMetrics.IR_METRICS)
        cols = [np.asarray(c, dtype=np.int64) for c in (columns, columns_other)]
        if sums.ndim != 2 or sums.shape[1] != q or any(c.ndim != 2 or c.shape != (cols[0].shape[0], q) for c in cols):
            raise ValueError(f"sums must be [n_perm, {q}] and both columns [U, {q}], got {sums.shape}, {cols[0].shape} and {cols[1].shape}")
        ta, tb = (c.astype(object).sum(axis=0) for c in cols)
        x = sums.astype(object)
        y = (ta + tb)[None, :] - x
        keep = np.asarray((x[:, 0] > 0) & (y[:, 0] > 0), dtype=bool)
        out = {"n_perm": int(len(sums)), "n_empty": int(np.sum(~keep)), "kept": int(np.sum(keep)), "seed": int(seed)}
        rx, ry = RetrievalMetrics._ir_ratios(x[keep]), RetrievalMetrics._ir_ratios(y[keep])
        if ta[0] == 0 or tb[0] == 0:
            return RetrievalMetrics._permutation_p_values(out, rx, ry, None, None, keep)
        return RetrievalMetrics._permutation_p_values(out, rx, ry, RetrievalMetrics._ir_ratios(ta), RetrievalMetrics._ir_ratios(tb), keep)

    @staticmethod
    def format_permutation(summary, prefix="", versus="raw"):
        """One line: every logged metric's signed difference and its two-sided p-value (a rank summary or an IR summary)."""
        if "median" in summary:
            label = {"R1": "R@1", "R5": "R@5", "R10": "R@10", "MedianR": "Median R", "MeanR": "Mean R"}
            names = [n for n in RetrievalMetrics.BOOTSTRAP_LOGGED if n in summary]
        else:
            label, names = RetrievalMetrics.IR_LABELS, list(RetrievalMetrics.IR_METRICS)
        parts = [f"{label[n]}: {summary[n]['diff']:+.2f} p={summary[n]['p_two']:.4f}" for n in names]
        tail = f" (paired permutation test vs {versus}, {summary['n_perm']} permutations"
        tail += f", {summary['n_empty']} empty)" if summary["n_empty"] else ")"
        return prefix + " - ".join(parts) + tail

    def log_permutation(self, summary, prefix="", versus="raw"):
        """One line per summary, in the style of print_metrics (silent without a logger)."""
        if self.logger is not None:
            self.logger.info(self.format_permutation(summary, prefix, versus))

    # ---- paired permutation test of hubness (DESIGN.md "Permutation test of hubness") ---------------------------------------------------
    HUBNESS_TEST_METRICS = ("skewness", "anti_hub_pct", "hub_pct", "bad_hub_pct", "hub_occurrence_pct", "good_occurrence_pct",
                            "max_occurrence")
    HUBNESS_TEST_LABELS = {"skewness": "skew", "anti_hub_pct": "anti-hubs", "hub_pct": "hubs", "bad_hub_pct": "bad hubs",
                           "hub_occurrence_pct": "hub occurrence", "good_occurrence_pct": "good occurrence", "max_occurrence": "max N_k"}

    @staticmethod
    def hubness_moments(occ, good):
        """int64 [9], the integers of ops.permtest_hubness for un-permuted k-occurrence counts occ = N and good = GN over the gallery:
        S1 = sum N, S2 = sum N^2, S3 = sum N^3, #{N = 0}, hubs = #{N G > 2 S1}, the sum of N over the hubs, #{hub and N - GN > GN},
        sum GN, max N."""
        occ = np.asarray(occ, dtype=np.int64).reshape(-1)
        good = np.asarray(good, dtype=np.int64).reshape(-1)
        if occ.shape != good.shape or occ.size == 0:
            raise ValueError("occ and good must be non-empty and of one length")
        s1 = int(occ.sum())
        hubs = occ * occ.size > 2 * s1
        return np.asarray([s1, int(np.sum(occ ** 2)), int(np.sum(occ ** 3)), int(np.sum(occ == 0)), int(np.sum(hubs)),
                           int(np.sum(occ[hubs])), int(np.sum(hubs & (occ - good > good))), int(good.sum()), int(occ.max())],
                          dtype=np.int64)

    @staticmethod
    def _hubness_skewness(m, G):
        """fp64 skewness of rows (S1, S2, S3, ...) of Python ints (object arrays): float(c) / (float(a) sqrt(float(a))) with
        a = G S2 - S1^2 and c = G^2 S3 - 3 G S1 S2 + 2 S1^3 taken exactly; 0.0 where a = 0."""
        s1, s2, s3 = m[..., 0], m[..., 1], m[..., 2]
        a = np.asarray(G * s2 - s1 * s1, dtype=object)
        c = np.asarray(G * G * s3 - 3 * G * s1 * s2 + 2 * s1 * s1 * s1, dtype=object)
        a, c = a.astype(np.float64), c.astype(np.float64)                      # float() of every exact integer: rounded once
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(a != 0, c / (a * np.sqrt(a)), 0.0)

    @staticmethod
    def _hubness_ratios(m, G):
        """{metric: (numerator, denominator)} of the six rational figures of rows of the nine integers (object arrays)."""
        one = 1 + 0 * m[..., 0]
        return {"anti_hub_pct": (100 * m[..., 3], G * one), "hub_pct": (100 * m[..., 4], G * one), "bad_hub_pct": (100 * m[..., 6], G * one),
                "hub_occurrence_pct": (100 * m[..., 5], m[..., 0]), "good_occurrence_pct": (100 * m[..., 7], m[..., 0]),
                "max_occurrence": (m[..., 8], one)}

    @staticmethod
    def hubness_permutation_summary(stats, moments_a, moments_b, n_gallery, seed=0):
        """Paired permutation (randomisation) test of the hubness of "ranking A minus ranking B": stats [n_perm, 2, 9] int64
        (ops.permtest_hubness: the sides X, Y of every relabelling), moments_a / moments_b = hubness_moments of the un-permuted A / B
        over the gallery of n_gallery items.  Per side: skewness (the formula of _hubness_skewness), anti_hub_pct = 100 anti / G,
        hub_pct, bad_hub_pct likewise, hub_occurrence_pct = 100 hub_occ / S1, good_occurrence_pct = 100 good / S1, max_occurrence.
        d_p = m(X_p) - m(Y_p), d_0 = m(A) - m(B); permutations with an empty side (S1 = 0) are dropped (n_empty).  -> {"n_perm",
        "n_empty", "kept", "seed", and per metric "diff", "p_two", "p_ge", "p_le" as permutation_summary}.  The six rational figures
        are compared on cross-multiplied Python integers; skewness is irrational and is compared in fp64: equal integers give equal
        doubles, and the mirror image of a relabelling gives exactly -d."""
        stats = np.asarray(stats.cpu() if torch.is_tensor(stats) else stats, dtype=np.int64)
        ma, mb = (np.asarray(m, dtype=np.int64).reshape(-1).astype(object) for m in (moments_a, moments_b))
        if stats.ndim != 3 or stats.shape[1:] != (2, 9) or ma.shape != (9,) or mb.shape != (9,):
            raise ValueError(f"stats must be [n_perm, 2, 9] and both moments [9], got {stats.shape}, {ma.shape} and {mb.shape}")
        G = int(n_gallery)
        if G < 1:
            raise ValueError(f"n_gallery must be positive, got {n_gallery!r}")
        keep = (stats[:, 0, 0] > 0) & (stats[:, 1, 0] > 0)
        kept = int(np.sum(keep))
        out = {"n_perm": int(len(stats)), "n_empty": int(np.sum(~keep)), "kept": kept, "seed": int(seed)}
        x, y = stats[keep, 0].astype(object), stats[keep, 1].astype(object)
        rx, ry = RetrievalMetrics._hubness_ratios(x, G), RetrievalMetrics._hubness_ratios(y, G)
        if ma[0] == 0 or mb[0] == 0:
            out["skewness"] = {"diff": float("nan"), "p_two": float("nan"), "p_ge": float("nan"), "p_le": float("nan")}
            return RetrievalMetrics._permutation_p_values(out, rx, ry, None, None, keep)
        d0 = float(RetrievalMetrics._hubness_skewness(ma, G) - RetrievalMetrics._hubness_skewness(mb, G))
        d = RetrievalMetrics._hubness_skewness(x, G) - RetrievalMetrics._hubness_skewness(y, G) if kept else np.zeros((0,))
        two, ge, le = int(np.sum(np.abs(d) >= abs(d0))), int(np.sum(d >= d0)), int(np.sum(d <= d0))
        out["skewness"] = {"diff": d0, "p_two": (1 + two) / (1 + kept), "p_ge": (1 + ge) / (1 + kept), "p_le": (1 + le) / (1 + kept)}
        return RetrievalMetrics._permutation_p_values(out, rx, ry, RetrievalMetrics._hubness_ratios(ma, G),
                                                      RetrievalMetrics._hubness_ratios(mb, G), keep)

    @staticmethod
    def format_hubness_permutation(summary, k, prefix="", versus="raw"):
        """One line: every hubness figure's signed difference and its two-sided p-value."""
        parts = [f"{RetrievalMetrics.HUBNESS_TEST_LABELS[n]} {summary[n]['diff']:+.2f} p={summary[n]['p_two']:.4f}"
                 for n in RetrievalMetrics.HUBNESS_TEST_METRICS]
        tail = f" (paired permutation test vs {versus}, {summary['n_perm']} permutations"
        tail += f", {summary['n_empty']} empty)" if summary["n_empty"] else ")"
        return f"{prefix}Hubness@{int(k)}: " + " - ".join(parts) + tail

    def log_hubness_permutation(self, summary, k, prefix="", versus="raw"):
        """One line per direction, in the style of log_permutation (silent without a logger)."""
        if self.logger is not None:
            self.logger.info(self.format_hubness_permutation(summary, k, prefix, versus))

    def print_metrics(self, metrics, prefix=""):
        msg = (f"{prefix}R@1: {metrics['R1']:.1f} - R@5: {metrics['R5']:.1f} - R@10: {metrics['R10']:.1f} - "
               f"R@50: {metrics.get('R50', 0.0):.1f} - Median R: {metrics['MR']:.1f} - Mean R: {metrics['MeanR']:.1f}")
        if self.logger is not None:                         # metrics.py:154: silent without a logger
            self.logger.info(msg)

    def update_best_metrics(self, t2v_metrics, v2t_metrics, t2v_r1=None, v2t_r1=None):
        """metrics.py:168-203: keep the best t2v / v2t R@1 seen so far (ties update too) -> (is_updated, mean R@1 now)."""
        t2v_r1 = t2v_metrics["R1"] if t2v_r1 is None else t2v_r1
        v2t_r1 = v2t_metrics["R1"] if v2t_r1 is None else v2t_r1
        is_updated = False
        if self.best_t2v_r1 <= t2v_r1:
            self.best_t2v_r1, self.best_t2v_metrics = t2v_r1, dict(t2v_metrics)
            self.best_mean_r1 = (self.best_t2v_r1 + self.best_v2t_r1) / 2
            is_updated = True
        if self.best_v2t_r1 <= v2t_r1:
            self.best_v2t_r1, self.best_v2t_metrics = v2t_r1, dict(v2t_metrics)
            self.best_mean_r1 = (self.best_t2v_r1 + self.best_v2t_r1) / 2
            is_updated = True
        return is_updated, (t2v_r1 + v2t_r1) / 2

    def log_current_metrics(self, t2v_metrics, v2t_metrics, mean_r1):
        if self.logger is None:
            return
        self.logger.info(f"Mean R@1: {mean_r1:.4f}")
        self.logger.info("Text-to-Video Retrieval:")
        self.print_metrics(t2v_metrics, prefix="  ")
        self.logger.info("Video-to-Text Retrieval:")
        self.print_metrics(v2t_metrics, prefix="  ")

    def log_best_metrics(self):
        if self.logger is None or self.best_t2v_metrics is None or self.best_v2t_metrics is None:
            return
        self.logger.info(f"Best Mean R@1: {self.best_mean_r1:.4f}")
        self.logger.info("Best Text-to-Video Retrieval:")
        self.print_metrics(self.best_t2v_metrics, prefix="  ")
        self.logger.info("Best Video-to-Text Retrieval:")
        self.print_metrics(self.best_v2t_metrics, prefix="  ")

    def get_best_metrics(self):
        return {"score": self.best_mean_r1, "text_to_video": self.best_t2v_metrics, "video_to_text": self.best_v2t_metrics,
                "t2v_r1": self.best_t2v_r1, "v2t_r1": self.best_v2t_r1}
