#!/usr/bin/env python
"""The kernels of nr_hubnorm.hip (row statistics, column partials, combine, the `is` and `dsl` applies) on an N x N fp32 slab, a
few launches each, for a rocprofv3 kernel trace: the evaluation's other profile tools launch none of them but the combine.

    rocprofv3 --kernel-trace --stats -f csv -d DIR -o run -- python tools/hubnorm_profile.py N [repeats]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(N, repeats):
    import torch
    from neighborretr_amd import ops
    g = torch.Generator(device="cuda").manual_seed(4242)
    S = torch.randn((N, N), generator=g, device="cuda") * 0.1
    for _ in range(repeats + 1):                                            # the first round is the warm-up
        row = ops.hubnorm_row_lse(S, 20.0)
        stats = ops.hubnorm_col_stats(S, 20.0)
        col = ops.hubnorm_combine(stats[None].contiguous())
        for mode in ("is", "dsl"):
            T, V = ops.hubnorm_apply(S, 20.0, mode, col_norm=col, row_norm=row)
    torch.cuda.synchronize()
    print(f"N = {N}: {repeats + 1} rounds of row_lse, col_stats, combine and both applies;  T[0, 0] = {float(T[0, 0]):.4f}")


if __name__ == "__main__":
    run(int(sys.argv[1]), int(sys.argv[2]) if len(sys.argv) > 2 else 20)
