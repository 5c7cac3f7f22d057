"""Times the exact brute-force searcher against torch matmul + topk.

    python tools/bench_brute_force.py [--shape configs0|glove|all] [--steps 20] [--warmup 3]
                                      [--out profiles/brute_force/bench.json]

smx_bf_search_batched_device with device-resident queries, at
  configs0  100k x 128 U[0,1) seed 1, batch 100, squared L2, k = 10
  glove     synthetic.glove_like() (1,183,514 x 100), batch 1000, dot, k = 10
and, in the same process, the baseline torch.topk(q @ db_chunk.T, k) in
float32 over row chunks that fit memory, merged across chunks.  Each is warmed
up, then timed per step by device events; the median is reported.  One JSON
line per shape: both times, QPS, the ratio, the searcher's passes /
fallback_pieces and frac_f32_mfma = 2 nq N dim / t / 155e12 (the whole call's
rate over the measured f32-MFMA rate: an end-to-end figure, not a kernel's).
The ids of both paths are compared (recall of the searcher's ids in the
baseline's; float32 GEMM rounding may swap near-ties)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

F32_MFMA_FLOPS = 155e12   # measured dense f32 MFMA rate of one MI355X


def shapes(which):
    from scann_amd import synthetic
    if which in ("configs0", "all"):
        rng = np.random.default_rng(1)
        yield ("configs0", rng.random((100000, 128), dtype=np.float32),
               rng.random((100, 128), dtype=np.float32), "squared_l2")
    if which in ("glove", "all"):
        db, q = synthetic.glove_like()
        yield "glove", db, q, "dot_product"


def time_steps(torch, stream, fn, steps, warmup):
    """(median, min, max) ms of fn()'s work on `stream`, by device events."""
    ms = []
    with torch.cuda.stream(stream):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        for _ in range(steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def baseline(torch, dbt, qt, k, metric, chunk):
    """topk(q @ chunk.T) per row chunk, merged: ids [nq][k]."""
    best_v = best_i = None
    for s in range(0, dbt.shape[0], chunk):
        xb = dbt[s:s + chunk]
        sc = qt @ xb.T
        if metric == "squared_l2":
            # |x|^2 - 2 q.x (|q|^2 does not change a query's order)
            sc = (xb * xb).sum(1)[None, :] - 2 * sc
            v, i = torch.topk(sc, min(k, sc.shape[1]), dim=1, largest=False)
        else:
            v, i = torch.topk(sc, min(k, sc.shape[1]), dim=1, largest=True)
        i = i + s
        if best_v is None:
            best_v, best_i = v, i
        else:
            av, ai = torch.cat([best_v, v], 1), torch.cat([best_i, i], 1)
            v2, o = torch.topk(av, k, dim=1, largest=metric != "squared_l2")
            best_v, best_i = v2, torch.gather(ai, 1, o)
    return best_i


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", choices=["configs0", "glove", "all"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--chunk", type=int, default=1 << 18, help="baseline rows per chunk")
    ap.add_argument("--out", default=None, help="also write the results as a JSON list")
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps must be at least 20 (the median of at least 20 steps)")

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_brute_force.py needs a GPU (no CPU fallback)")
    from scann_amd import _native
    from scann_amd.brute_force import BruteForceIndex
    from scann_amd.index import METRIC_NAMES

    results = []
    # one explicit stream for both paths (the library is handed the same one)
    stream = torch.cuda.Stream()
    sptr = ctypes.c_void_p(stream.cuda_stream)
    for name, db, q, metric in shapes(args.shape):
        nq, dim = q.shape
        n, k = db.shape[0], args.k
        bf = _native.NativeBruteForce(BruteForceIndex(db, METRIC_NAMES[metric]), device=0)
        qt = torch.from_numpy(q).cuda()
        oi = torch.zeros((nq, k), dtype=torch.int32, device="cuda")
        od = torch.zeros((nq, k), dtype=torch.float32, device="cuda")

        def ours():
            bf.search_batched_device(qt.data_ptr(), nq, k, oi.data_ptr(), od.data_ptr(), stream=sptr)

        t_ours = time_steps(torch, stream, ours, args.steps, args.warmup)
        stats = bf.stats()
        ids_ours = oi.cpu().numpy().astype(np.int64)
        bf.close()

        dbt = torch.from_numpy(db).cuda()
        ids_base = None

        def base():
            nonlocal ids_base
            ids_base = baseline(torch, dbt, qt, k, metric, args.chunk)

        t_base = time_steps(torch, stream, base, args.steps, args.warmup)
        ib = ids_base.cpu().numpy()
        agree = float(np.mean([len(set(a) & set(b)) / k for a, b in zip(ids_ours.tolist(), ib.tolist())]))
        del dbt
        torch.cuda.empty_cache()
        t = t_ours[0] * 1e-3
        res = dict(shape=name, n=int(n), dim=int(dim), nq=int(nq), k=int(k), metric=metric,
                   steps=args.steps, warmup=args.warmup,
                   brute_force_ms=round(t_ours[0], 4), brute_force_ms_min=round(t_ours[1], 4),
                   brute_force_ms_max=round(t_ours[2], 4),
                   torch_ms=round(t_base[0], 4), torch_ms_min=round(t_base[1], 4),
                   torch_ms_max=round(t_base[2], 4), torch_chunk_rows=args.chunk,
                   ratio_torch_over_brute_force=round(t_base[0] / t_ours[0], 3),
                   qps=round(nq / t, 1), torch_qps=round(nq / (t_base[0] * 1e-3), 1),
                   passes=stats["passes"], fallback_pieces=stats["fallback_pieces"],
                   max_candidates=stats["max_candidates"],
                   frac_f32_mfma=round(2.0 * nq * n * dim / t / F32_MFMA_FLOPS, 4),
                   id_agreement_with_torch=round(agree, 5))
        print(json.dumps(res), flush=True)
        results.append(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
