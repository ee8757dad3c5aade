#!/usr/bin/env python3
"""Headline benchmark: acquisition evals/sec (+ GP-fit ms) at N=2048, D=20, M=65536.

One "step" = one pass of the candidate-scoring hot path over one batch of M synthetic
candidates already resident in HBM: K* build + posterior mean (K2+K3), posterior variance
through the fp64-MFMA quadratic form (K4), pointwise-EI score and the on-device argmax,
plus (N>1) one RCCL all-gather of the 16-byte (score, index) record.

    python bench.py                                   # C3, 1 GPU
    python bench.py --gpus 8                          # spawns 8 ranks itself (torch.distributed.run)
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...   # the driver's form
    python bench.py --gpus 8 --config c4              # BASELINE config 4: 262144 candidates SHARDED over the ranks

--scaling strong (default): --candidates is the JOB total -- BASELINE's metric is quoted at a fixed M (C3: 65536) on
1/2/4/8 GPUs -- and rank r scores rows shard_bounds(M, r, N); `value` is that strong-scaling rate.  With more than one
rank the same line also carries `weak_scaling_leg`: every rank scoring its own --candidates rows (timed right after).
--scaling weak makes the weak leg the headline instead.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_FP64_MFMA_TFLOPS = 78.6   # MI355X dense fp64 matrix peak (public spec)
PEAK_HBM_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec


def synth_model_inputs(cfg):
    """Design X / f_init for the workload.  The committed fixture holds the design the reference's own
    FeedbackProcessing produced for this recipe (seed 0, m=31); nothing is read from /root/reference."""
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", f"{cfg}.npz")))
    return g


def cpu_baseline(g, M_sample, seconds_budget=25.0, gpu_check=None):
    """Oracle (CPU restatement of the reference) timed on the host cores on a bounded sample."""
    from oracle import ppbo_oracle as orc
    import threadpoolctl
    X, th, m, kern = g["X"], g["theta"], int(g["m"]), str(g["kernel"])
    D = X.shape[1]
    Sinv = orc.pd_inverse(orc.gram(X, th, kern))
    f = g["fMAP"]
    P = orc.posterior_covariance(Sinv, f, m, th[0])
    A = orc.variance_operator(Sinv, P, faithful=False, lam=orc.lambda_dense(f, m, th[0]))
    alpha = Sinv @ f
    Xc = np.random.default_rng(1).random((M_sample, D))
    mustar = float(np.max(g["mu"]))
    # optimised-CPU mode: cached alpha / A, batched GEMM scoring
    t0 = time.perf_counter()
    reps = 0
    while True:
        mu, var = orc.predict_mean_var(Xc, X, th, alpha, A, kern)
        sc = orc.pointwise_ei(mu, var, mustar)
        _ = int(np.argmax(sc))
        reps += 1
        if time.perf_counter() - t0 > seconds_budget * 0.6 or reps >= 20:
            break
    opt_rate = reps * M_sample / (time.perf_counter() - t0)
    # faithful-cost mode: (k' Sigma^-1) f per candidate, as mu_pred does (gp_model.py:454-458)
    n_f = 0
    t1 = time.perf_counter()
    while time.perf_counter() - t1 < seconds_budget * 0.4 and n_f < 4096:
        orc.mu_pred(Xc[n_f % M_sample], X, th, Sinv, f, kern)
        n_f += 1
    faithful_rate = n_f / (time.perf_counter() - t1)
    # GP fit on the CPU, the reference's way: Sigma (closed-form shrink), posv inverse, SciPy trust-exact from the
    # same start vector, Lambda and the posterior covariance (gp_model.py:91-117)
    tf = time.perf_counter()
    Sg = orc.gram(X, th, kern)
    Si = orc.pd_inverse(Sg)
    fm, _ = orc.fit_fmap_trust_exact(g["f_init"], Si, m, th[0])
    _ = orc.posterior_covariance(Si, fm, m, th[0])
    cpu_fit_ms = (time.perf_counter() - tf) * 1e3
    parity = None
    if gpu_check is not None:   # in-situ parity of the timed path against the oracle on a subsample
        Xs, mu_gpu, var_gpu = gpu_check
        mu_o, var_o = orc.predict_mean_var(Xs, X, th, alpha, A, kern)
        parity = {"candidates": int(Xs.shape[0]),
                  "mu_max_rel_err": float(np.max(np.abs(mu_gpu - mu_o)) / np.max(np.abs(mu_o))),
                  "var_max_err_over_sf2": float(np.max(np.abs(var_gpu - var_o)) / float(th[2]) ** 2),
                  "tolerance": 1e-5}
    info = threadpoolctl.threadpool_info()
    nthreads = max([i.get("num_threads", 1) for i in info] + [1])
    return dict(value=opt_rate, unit="evals/s", cores=int(nthreads), kind="port",
                sample=f"{reps}x{M_sample} candidates mean+var+EI+argmax, cached alpha/A (optimised-CPU mode); "
                       f"faithful mu_pred per candidate: {faithful_rate:.0f} evals/s over {n_f} candidates",
                faithful_mu_pred_evals_per_s=faithful_rate, host_cpus=os.cpu_count(), gp_fit_ms=cpu_fit_ms,
                parity_vs_oracle=parity)



def c1_loop(torch):
    """BASELINE config 1 end to end: six-hump camel (D = 2), 4 corner initial queries + 21 PCD queries, m = 25 (the
    reference's default star size: N grows 26 -> 650), theta = [0.01, 0.26, 0.1], seed 0, through run_ppbo_loop (the loop
    of ppbo_numerical_main.py:57-144 on the drop-in classes).  The reference itself on 8 host cores: 81.4 s, final x*
    0.065 from the optimum (it cannot run on the GPU box)."""
    from ppbo_amd.misc import hypercube_corners
    from ppbo_amd.numerical_main import line_search_user, run_ppbo_loop
    from ppbo_amd.ppbo_settings import PPBO_settings

    def six_hump(v):
        x, y = v[..., 0], v[..., 1]
        return (4 - 2.1 * x ** 2 + x ** 4 / 3) * x ** 2 + x * y + (-4 + 4 * y ** 2) * y ** 2
    bounds = ((-3, 3), (-2, 2))
    lo, hi = np.array([-3.0, -2.0]), np.array([3.0, 2.0])
    out = {}
    for rep in range(2):          # the second run is the timed one (workspaces allocated, kernels loaded)
        np.random.seed(0)
        st = PPBO_settings(D=2, bounds=bounds, xi_acquisition_function="PCD", m=25, theta_initial=[0.01, 0.26, 0.1],
                           verbose=False)
        xis = np.tile(np.diag(hi), (2, 1))
        xs = hypercube_corners(bounds)[:4].astype(float)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        results, xstars, mustars, gp = run_ppbo_loop(line_search_user(six_hump, lo, hi), xis, xs, 21, st)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        opt = np.array([[0.0898, -0.7126], [-0.0898, 0.7126]])
        out = {"wall_s": dt, "queries": int(results.shape[0]), "N_final": int(gp.N), "m": 25,
               "final_xstar": [float(v) for v in xstars[-1]],
               "distance_to_optimum": float(np.min(np.linalg.norm(opt - xstars[-1][None, :], axis=1))),
               "f_at_xstar": float(six_hump(xstars[-1])),
               "reference_wall_s_8_host_cores": 81.4, "reference_distance_to_optimum": 0.065,
               "note": "the user is simulated by a line search on the objective, as the reference's pp_sixhump_camel does; "
                       "the last update runs the reference's 3 mu_star trials per iteration"}
    return out


def per_query_breakdown(torch, cfg="c2", reps=5):
    """One PPBO iteration on the shape of BASELINE config `cfg` (c2: D = 6, N = 512; c3: D = 20, N = 2048 -- the
    metric's shape) through the drop-in objects, phase by phase (ms, median of `reps`): what GPModel.update_model +
    next_query cost per query (ppbo_numerical_main.py:86-92,107-124).
      update_model_fit   the default update (one prior-draw start) = ONE ppbo_gp_fit call: Sigma, factor, inverse,
                         whitened f_MAP search, posterior (src/gp_model.py:91-117, without mu_star)
      fit_incremental    the same after ONE appended query with GPModel(incremental=True) (bordered factor, warm start)
      mu_star            per trial of the device-resident search (4 trials in one ppbo_mean_search_multi enqueue / 4;
                         the reference's default is 3 per iteration)
      update_model       GPModel.update_model() as the loop calls it: the fit + 3 mu_star trials
      next_query_*       every strategy family of src/acquisition.py:9-65: EI-EXT-FAST (D lines), EI-EXT (50 D lines),
                         EI / EXR (joint searches, BO_maxiter = 20), EI-VARMAX (50 D lines + the x search)
      hsampler_cycle     Hsampler(gp, F): basis, Phi(X), omega_MAP, one posterior sample and its maximiser
                         (src/random_fourier_sampler.py; the sequence of ppbo_numerical_main.py:279-292)"""
    from ppbo_amd.acquisition import next_query
    from ppbo_amd.gp_model import GPModel
    from ppbo_amd.ppbo_settings import PPBO_settings
    from ppbo_amd.random_fourier_sampler import Hsampler
    g = synth_model_inputs(cfg)
    D, m = int(g["D"]), int(g["m"])

    def model(acq, n_q, incremental=False):
        st = PPBO_settings(D=D, bounds=tuple(map(tuple, g["bounds"])), xi_acquisition_function=acq,
                           theta_initial=list(map(float, g["theta"])), m=m, verbose=False, kernel=str(g["kernel"]))
        gp = GPModel(st, incremental=incremental)
        np.random.seed(0)
        gp.update_feedback_processing_object(g["X_obs"][:n_q])
        gp.update_data()
        gp.turn_initialization_off()
        return gp, st

    def med(fn, n=reps):
        ts = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))

    n_q = g["X_obs"].shape[0]
    gp, st = model("EI-EXT-FAST", n_q)
    gp.set_theta()
    np.random.seed(1)
    assert gp._fit_fused()
    out = {"shape": f"{cfg}: N={gp.N}, D={D}, m={m}, theta={list(map(float, g['theta']))}"}
    out["update_model_fit_ms"] = med(lambda: gp._fit_fused())
    out["update_model_fit_lbfgs_evals"] = gp.fit_log[-1]["lbfgs_evals"]
    gp.mu_star(mustar_finding_trials=1)
    out["mu_star_ms_per_trial"] = med(lambda: gp.mu_star(mustar_finding_trials=4)) / 4.0
    gp.xstar, gp.mustar, gp.xstars_local = gp.mu_star()
    # the whole update of a query as the loop calls it: the fit + the reference's default 3 mu_star trials
    out["update_model_ms"] = med(lambda: gp.update_model())
    for acq, key in (("EI-EXT-FAST", "next_query_EI_EXT_FAST_ms"), ("EI-EXT", "next_query_EI_EXT_ms"),
                     ("EI", "next_query_EI_search_ms"), ("EXR", "next_query_EXR_search_ms"),
                     ("EI-VARMAX", "next_query_EI_VARMAX_ms")):
        sa = PPBO_settings(D=D, bounds=tuple(map(tuple, g["bounds"])), xi_acquisition_function=acq,
                           theta_initial=list(map(float, g["theta"])), m=m, verbose=False, kernel=str(g["kernel"]))
        next_query(sa, gp)
        out[key] = med(lambda: next_query(sa, gp), 3)
    if str(g["kernel"]) == "SE_kernel":          # the reference has a spectral basis for the SE kernel only
        F = 4096 if cfg == "c3" else 1000

        def cycle():
            hs = Hsampler(gp, F)
            hs.generate_basis()
            hs.update_phi_X()
            hs.update_omega_MAP()
            hs.update_covariancematrix()
            hs.sample_xstar()
        cycle()
        out["hsampler_cycle_ms"] = med(cycle, 3)
        out["hsampler_features"] = F
    # incremental: fit n_q - 1 queries, then time the update that appends the last one
    ts = []
    for _ in range(3):
        gi, _ = model("PCD", n_q - 1, incremental=True)
        np.random.seed(2)
        gi.update_model()
        gi.update_feedback_processing_object(g["X_obs"][:n_q])
        gi.update_data()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gi.update_Sigma(gi.theta)
        gi.update_Sigma_inv(gi.theta)
        gi.update_fMAP()
        gi._post = gi.eng.posterior(gi._dX, gi.theta, gi.kernel.__name__, gi._dSigma_inv, gi.eng.dev(gi.fMAP), gi.m)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
        assert gi.n_appends == 1
    out["fit_incremental_ms"] = float(np.median(ts))
    out["fit_incremental_cholesky"] = gi.fit_log[-1]["n_cholesky"]
    return out

# BASELINE.json configs that have a committed design fixture: name, default candidate count, default scaling
WORKLOADS = {
    "c2": ("C2 Hartmann6-shaped", 16384, "strong"),
    "c3": ("C3 Ackley-shaped", 65536, "strong"),
    "c4": ("C4 Levy-shaped", 262144, "strong"),
    "c5": ("C5 camphor/Cu(111)-shaped", 65536, "strong"),
}


def other_config_row(torch, eng, cfg, steps=20):
    """One BASELINE configuration other than the headline one, measured inside the default run so that the DRIVER's clock
    covers it: the cold fit (median of three after a warm-up) and `steps` scoring steps of the config's own
    candidate count on this GPU, with the dominant kernel's executed-flops fraction of the fp64 MFMA peak."""
    from ppbo_amd.dist import ShardedSearch
    from ppbo_amd.engine import SCORE_POINTWISE_EI
    g = synth_model_inputs(cfg)
    X, th, m, kern = g["X"], g["theta"], int(g["m"]), str(g["kernel"])
    N, D = X.shape
    M = WORKLOADS[cfg][1]
    Xd = eng.dev(X)
    if bool(g.get("f_init_is_warm_start", False)):
        Ls = eng.potrf_(eng.gram(Xd, th, kern).clone())
        f_init = eng.dgemv(Ls, np.random.default_rng(2).standard_normal(N), lower=True)
        del Ls
    else:
        f_init = eng.dev(g["f_init"])
    fit = lambda: eng.gp_fit(Xd, th, kern, m, f_init, gtol=1e-4, start_is_whitened=False)
    r = fit()
    torch.cuda.synchronize()
    runs = []
    for _ in range(3):
        t0 = time.perf_counter()
        r = fit()
        torch.cuda.synchronize()
        runs.append((time.perf_counter() - t0) * 1e3)
    post = r["post"]
    Xc = eng.dev(np.random.default_rng(1).random((M, D)))
    mustar = float(np.max(g["mu"]))
    search = ShardedSearch(eng, post, Xc, 0, SCORE_POINTWISE_EI, mustar)
    for _ in range(3):
        search.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        search.step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    eng.profile(True)
    for _ in range(5):
        search.step()
    torch.cuda.synchronize()
    qf, qn = eng.profile_read("quadform")
    fu, fn_ = eng.profile_read("fused_score")
    ks, kn = eng.profile_read("kstar")
    eng.profile(False)
    fused = fn_ > 0 and qn == 0
    mblk = m + 1
    launches_per_step = 1 if fused else max(1, -(-M // 65536))
    M_launch = float(M) / launches_per_step
    exec_flops = sum(2.0 * 32 * M_launch * min(N, -(-((b + 1) * 32) // mblk) * mblk) for b in range(-(-N // 32)))
    k_ms = (fu / max(fn_, 1)) if fused else qf / max(qn, 1)
    del search, Xc, post, r
    return {"workload": WORKLOADS[cfg][0], "N": N, "D": D, "M": M, "ms_per_step": dt * 1e3, "evals_per_s": M / dt,
            "gp_fit_ms_from_f_init": float(np.median(runs)),
            "dominant_kernel": "fused_score_kernel (one launch: K* in LDS + contraction + score)" if fused else "quadform_kernel",
            "dominant_kernel_ms": k_ms, "launches_per_step": launches_per_step,
            "frac_of_fp64_mfma_peak": exec_flops / (k_ms * 1e-3) / 1e12 / PEAK_FP64_MFMA_TFLOPS,
            "kstar_kernel_ms": None if fused else ks / max(kn, 1)}


def spawn_ranks(args) -> int:
    """`python bench.py --gpus N` outside torchrun: start N rank processes (one per GPU, RCCL) as a CHILD job and
    relay its output.  Nothing in this parent has touched HIP (torch is not even imported), so no process that
    initialised a GPU is ever replaced or forked."""
    import socket
    import subprocess
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="c3", choices=sorted(WORKLOADS),
                    help="design fixture to fit (c3 = Ackley-shaped N=2048, D=20: the configuration the metric is quoted on)")
    ap.add_argument("--candidates", type=int, default=0, help="0 = the config's own M (c3: 65536, c4: 262144 ...)")
    ap.add_argument("--scaling", choices=["weak", "strong"], default=None,
                    help="strong (default): --candidates in total, sharded over the ranks; weak: --candidates per rank")
    ap.add_argument("--collective", choices=["torch", "capi"], default="torch",
                    help="torch: torch.distributed all_gather_into_tensor (nccl = RCCL) on device records + ppbo_argmax_combine; "
                         "capi: the library's own RCCL communicator, one ppbo_search_sharded call per step")
    ap.add_argument("--force-dist", action="store_true",
                    help="initialise torch.distributed (nccl) and run the collective path even with ONE rank")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-secondary", action="store_true", help="skip the RFF / line-acquisition side measurements")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="skip the secondary rows config_c2 / _c4 / _c5 (counter passes: every hot kernel of the run then has "
                         "ONE benchmark-shaped launch size)")
    ap.add_argument("--no-precision-report", action="store_true",
                    help="skip the fp64 / fp32-K* report on the fixture's 512 candidates (with --no-secondary and "
                         "--no-cpu-baseline every kernel row of a rocprofv3 --stats run is then ONE launch shape)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned (the job-wide best score and its "
                         "global candidate row) as DIR/best_score.npy and DIR/best_index.npy, float64; the inputs are seeded, "
                         "so two builds run with the same arguments can be compared output for output")
    args = ap.parse_args()
    if args.gpus < 1:
        ap.error("--gpus must be >= 1")
    if args.steps < 1:
        ap.error("--steps must be >= 1 (ms_per_step is the time of one timed step)")
    if args.warmup < 0:
        ap.error("--warmup must be >= 0")
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(spawn_ranks(args))

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: launch with --nproc-per-node {args.gpus} "
                 f"(or run `python bench.py --gpus {args.gpus}` without torchrun and let it spawn the ranks)")
    if world > 1:
        # the side measurements (RFF, line acquisitions, per-query breakdown, precision report, cpu_baseline) belong to
        # the N = 1 line: with several ranks they would keep rank 0 busy for half a minute while the others wait in
        # destroy_process_group
        args.no_secondary = args.no_precision_report = args.no_cpu_baseline = True
    wl_name, m_default, scaling_default = WORKLOADS[args.config]
    scaling = args.scaling or scaling_default
    M_arg = args.candidates or m_default

    # before anything touches HIP: the host driver only supports dmabuf IPC (RCCL needs it), rendezvous on loopback
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")

    import torch
    import torch.distributed as dist
    from ppbo_amd.engine import Engine, SCORE_POINTWISE_EI
    from ppbo_amd.dist import ShardedSearch, shard_bounds

    if not torch.cuda.is_available():
        sys.exit("bench.py: no ROCm GPU visible (torch.cuda.is_available() is False); the product has no CPU path")
    # PPBO_BENCH_SHARE_GPU=1 (tests only): every rank uses cuda:0 and the collectives run over gloo on host
    # tensors -- RCCL refuses two ranks on one device, and this build environment only has 1-GPU boxes; it
    # exercises the whole multi-rank control flow (sharding, barriers, max-over-ranks timing, the argmax exchange)
    share_gpu = os.environ.get("PPBO_BENCH_SHARE_GPU") == "1"
    gpu_index = 0 if share_gpu else local_rank
    use_dist = world > 1 or args.force_dist
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if "MASTER_PORT" not in os.environ:        # --force-dist outside torchrun: a free loopback port
            import socket
            with socket.socket() as so:
                so.bind(("127.0.0.1", 0))
                os.environ["MASTER_PORT"] = str(so.getsockname()[1])
        torch.cuda.set_device(gpu_index)
        if share_gpu:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world,
                                    device_id=torch.device("cuda", local_rank))
    eng = Engine(gpu_index)
    dev = eng.device
    coll_dev = torch.device("cpu") if share_gpu else dev       # where the collectives' tensors live

    g = synth_model_inputs(args.config)
    X, th, m, kern = g["X"], g["theta"], int(g["m"]), str(g["kernel"])
    N, D = X.shape
    if scaling == "strong":      # the job scores M_arg candidates in total; this rank owns a contiguous row block
        row_lo, row_hi = shard_bounds(M_arg, rank, world)
        M_total = M_arg
    else:                        # every rank scores M_arg candidates of its own
        row_lo, row_hi = rank * M_arg, (rank + 1) * M_arg
        M_total = M_arg * world
    M = row_hi - row_lo

    # ---- GP fit (untimed for the step metric, reported as gp_fit_ms) -------------------
    Xd = eng.dev(X)
    f_init = eng.dev(g["f_init"])
    fit_start = "the fixture's stored prior draw (default_rng(2), SURVEY 8d)"
    if bool(g.get("f_init_is_warm_start", False)):
        # C5's stored start is a near-optimal vector (the reference's own cold fit takes > 15 h): time the COLD fit from
        # a prior draw L z instead, as tools/c5_start.py / tests/test_gpu_c5.py do
        Ls = eng.potrf_(eng.gram(Xd, th, kern).clone())
        f_init = eng.dgemv(Ls, np.random.default_rng(2).standard_normal(N), lower=True)
        del Ls
        fit_start = "prior draw L z, z = default_rng(2) (the fixture's own start is a warm start)"
    # the start in the whitened variable, z0 = L^-1 f_init (untimed): ppbo_gp_fit takes it as the drop-in's update_model
    # hands it over (GPModel._fit_fused draws z0 ~ N(0, I) itself and starts from the prior draw L z0), which is also
    # what lets the call overlap the triangular inverse and Sigma^-1 with the first evaluations of the search
    _, Linv0, _ = eng.pd_inverse_factors3(eng.gram(Xd, th, kern))
    z_init = eng.dgemv(Linv0, f_init, lower=True)
    del Linv0
    fit_start += "; passed as z0 = L^-1 f_init (start_is_whitened)"
    def fit_once(whitened=True):
        """Sigma, Sigma^-1 (+ the Cholesky factor), f_MAP from the stored start, Lambda_MAP / G: the work of
        update_Sigma + update_Sigma_inv + update_fMAP(1 trial) + the posterior (src/gp_model.py:91-117).
        whitened=True: ONE library call (ppbo_gp_fit: everything enqueued on one stream, one host wait);
        whitened=False: the exact trust-region Newton on f alone (rounds 1-2's fit), call by call, timed beside it."""
        if whitened:
            r = eng.gp_fit(Xd, th, kern, m, z_init, gtol=1e-4, start_is_whitened=True)
            return r["post"], r["stats"]
        Sigma = eng.gram(Xd, th, kern)
        Sinv = eng.pd_inverse(Sigma)
        fmap, st = eng.fit_fmap(Sinv, f_init, m, th[0], gtol=1e-4, L=None)
        post = eng.posterior(Xd, th, kern, Sinv, fmap, m)
        return post, st
    def fit_from_f_init():
        """The protocol's fit ('timed end to end with the stored f_init'): the SAME library call
        handed f_init itself -- nothing precomputed outside the timed call; the library whitens it with the factor's
        inverse (z0 = L^-1 f_init), so the search's stream waits for the triangular inverse before its first evaluation
        instead of running beside it."""
        r = eng.gp_fit(Xd, th, kern, m, f_init, gtol=1e-4, start_is_whitened=False)
        return r["post"], r["stats"]
    post, st = fit_once()            # warm-up (allocates workspaces)
    torch.cuda.synchronize()
    n_fit = 5 if N <= 2048 else 3    # one warm-up, then the MEDIAN of five runs (three beyond N = 2048)
    fit_runs = []
    for _ in range(n_fit):           # the same deterministic cold fit every time
        t0 = time.perf_counter()
        post, st = fit_once()
        torch.cuda.synchronize()
        fit_runs.append((time.perf_counter() - t0) * 1e3)
    gp_fit_ms = float(np.median(fit_runs))
    fit_from_f_init()                # warm-up of the other start kind
    torch.cuda.synchronize()
    fit_runs_f = []
    for _ in range(n_fit):
        t0 = time.perf_counter()
        _, st_f = fit_from_f_init()
        torch.cuda.synchronize()
        fit_runs_f.append((time.perf_counter() - t0) * 1e3)
    gp_fit_ms_from_f_init = float(np.median(fit_runs_f))
    eng.profile(True)                # one more fit with the library's event brackets: where the fit time goes
    fit_once()
    torch.cuda.synchronize()
    potrf_ms, potrf_n = eng.profile_read("potrf")
    eng.profile(False)
    # the same fit through the exact trust-region Newton on f alone (what rounds 1-2 shipped): how much the
    # whitened search buys, on this box, in this run (rank 0 only; skipped beyond N = 2048 where it takes seconds)
    tr_fit_ms, tr_st = None, None
    if rank == 0 and N <= 2048:
        fit_once(whitened=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, tr_st = fit_once(whitened=False)
        torch.cuda.synchronize()
        tr_fit_ms = (time.perf_counter() - t0) * 1e3
    # (e) the model state is REPLICATED by running the same deterministic fit on every rank (no broadcast): check it --
    # an exact checksum (int64 view, wrapping sum) of alpha and G per rank, gathered; must be bitwise equal
    replicated_equal = None
    if world > 1:
        chk = torch.stack([post.alpha.view(torch.int64).sum(), post.G.view(torch.int64).sum()]).to(coll_dev)
        allchk = torch.empty(2 * world, dtype=torch.int64, device=coll_dev)
        dist.all_gather_into_tensor(allchk, chk)
        allchk = allchk.cpu().view(world, 2)
        replicated_equal = bool((allchk == allchk[0:1]).all())
        if not replicated_equal and rank == 0:
            print(f"bench.py: replicated fits differ between ranks: {allchk.tolist()}", file=sys.stderr)

    def burst_ms(fn, reps=40):
        """Steady-state duration of one launch of a SHORT kernel (8-100 us).  100 launches are captured in a HIP graph
        (torch.cuda.CUDAGraph over the stream the C-ABI launches on) and the graph is replayed back to back for tens
        of milliseconds, so that (a) the host's launch rate is out of the picture -- Python + ctypes issue one
        launch per ~17 us, which IS the duration of these kernels -- and (b) the clocks have settled under the
        kernel's own load (after an idle spell or a spin kernel the same kernel runs ~10 % slower, after half a
        second of fp64 MFMA work ~30 % slower: tools/alloc_effect.py, tools/dev/rff_ctx_effect.py).  The last half
        of the replays is timed with one event pair."""
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        try:
            if world > 1:       # never capture while an RCCL watchdog thread is polling events in this process
                raise RuntimeError("multi-rank run")
            per_graph, replays = max(10, min(100, reps * 2)), 40
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side):
                fn()
                torch.cuda.synchronize()
                with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
                    for _ in range(per_graph):
                        fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for r in range(replays):
                if r == replays // 2:
                    e0.record()
                graph.replay()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / ((replays - replays // 2) * per_graph)
        except Exception as exc:      # noqa: BLE001  -- graph capture unavailable: plain burst behind a blocker kernel
            if world == 1:
                print(f"bench.py: HIP-graph capture failed ({exc!r}); timing a plain burst instead", file=sys.stderr)
            torch.cuda.synchronize()
            if hasattr(torch.cuda, "_sleep"):
                torch.cuda._sleep(40_000_000)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / reps

    INFINITY_CACHE_BYTES = 256 * 2 ** 20     # MI355X: outputs below this are absorbed by the Infinity Cache, not HBM

    def gram_burst(Xg, reps=40):
        """Steady-state Gram time at this N, twice, plus the chip's write-only floor measured the same way:
        resident  -- every launch writes the SAME output buffer: up to N = 4096 (134 MB) that buffer lives in the 256 MB
                     Infinity Cache, so the figure is a fabric / last-level-cache write rate, NOT an HBM rate;
        streaming -- the launches rotate over enough output buffers that the replay's footprint exceeds 512 MB: every
                     byte has to reach HBM; this is the number the 8 TB/s roofline applies to;
        floor     -- ppbo_store_floor (write-only 32 x 128 tiles, 16-byte write-through stores) over the same rotating
                     buffers: the ceiling of any Gram kernel at this N on this chip, measured in this run."""
        Ng = Xg.shape[0]
        nbytes = 8 * Ng * Ng
        nbuf = max(1, -(-(2 * INFINITY_CACHE_BYTES) // nbytes))
        bufs = [eng.empty(Ng, Ng) for _ in range(nbuf)]
        state = {"k": 0}

        def rot(fn):
            def call():
                state["k"] = (state["k"] + 1) % nbuf
                fn(bufs[state["k"]])
            return call
        res = burst_ms(lambda: eng.gram(Xg, th, kern, out=bufs[0]), reps)
        stream = res if nbuf == 1 else burst_ms(rot(lambda o: eng.gram(Xg, th, kern, out=o)), reps)
        floor = burst_ms(rot(lambda o: eng.store_floor(o)), reps)
        gb = 8.0 * Ng * Ng + 8.0 * Ng * D
        rate = lambda ms: gb / (ms * 1e-3) / 1e9
        return {"N": Ng, "bytes": gb, "output_buffers_rotated": nbuf,
                "resident_ms": res, "resident_GBs": rate(res), "resident_frac_of_8TBs": rate(res) / PEAK_HBM_GBS,
                "resident_is_hbm": nbytes > INFINITY_CACHE_BYTES,
                "streaming_ms": stream, "streaming_GBs": rate(stream), "frac": rate(stream) / PEAK_HBM_GBS,
                "write_only_floor_ms": floor, "write_only_floor_frac": (8.0 * Ng * Ng) / (floor * 1e-3) / 1e9 / PEAK_HBM_GBS,
                "frac_of_floor": floor / stream}

    # ---- candidates resident in HBM ----------------------------------------------------
    if scaling == "strong":      # ONE job-wide candidate set (default_rng(1)); this rank holds its row block
        Xc = eng.dev(np.random.default_rng(1).random((M_arg, D))[row_lo:row_hi])
    else:
        Xc = eng.dev(np.random.default_rng(1 + rank).random((M, D)))
    mustar = float(np.max(g["mu"]))

    # ---- steady-state rates of the HBM-bound kernels (rank 0), each under its own load (see burst_ms) ---------
    gram_c3, gram_sizes, pj_burst_ms = None, {}, None
    F_RFF = 4096
    if rank == 0:
        gram_c3 = gram_burst(Xd)
    if rank == 0 and not args.no_secondary:
        W_rff = eng.dev(np.random.default_rng(3).standard_normal((F_RFF, D)) / th[1])
        b_rff = eng.dev(np.random.default_rng(4).uniform(0, 2 * np.pi, F_RFF))
        Phi_out = eng.empty(F_RFF, N)
        pj_burst_ms = burst_ms(lambda: eng.rff_project(Xd, W_rff, b_rff, th[2], out=Phi_out))
        del Phi_out
        for Ng in (4096, 8192):   # the Gram roofline is only meaningful beyond the launch-latency regime
            Xg = eng.dev(np.random.default_rng(7).random((Ng, D)))
            gram_sizes[str(Ng)] = gram_burst(Xg, 20)
            del Xg
    # ---- the timed region: K steps of the sharded search, nothing else -------------------------------------
    # A step = score this rank's rows (kstar, quadform, score + its own argmax: three launches), all-gather the
    # 16-byte device records, reduce, read ONE record back.  The persistent tensors live in `search`; the library's
    # event brackets are OFF here (they cost a few us per step) -- the per-kernel durations come from an identical
    # bracketed pass right after.
    search = ShardedSearch(eng, post, Xc, row_lo, SCORE_POINTWISE_EI, mustar, collective=args.collective,
                           host_collective=share_gpu)

    if use_dist:
        search.step()       # the communicator's lazy connection set-up belongs to the job's start, not to the first timed
                            # step of a --warmup 0 run

    def timed_steps(srch, steps, after_warmup=None):
        for _ in range(args.warmup):
            srch.step()
        if after_warmup is not None:
            after_warmup()
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            res = srch.step()
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
        dt = time.perf_counter() - t0
        if use_dist:
            tt = torch.tensor([dt], dtype=torch.float64, device=coll_dev)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            dt = float(tt.item())
        return dt, res

    elapsed, best = timed_steps(search, args.steps)
    # the same steps again with the library's HIP-event brackets on (on the stream the kernels are launched on): the
    # live per-kernel durations behind `roofline`; its wall time is reported beside the unbracketed one
    eng.profile(True)
    elapsed_bracketed, _ = timed_steps(search, args.steps, after_warmup=eng.profile_reset)
    qf_ms, qf_n = eng.profile_read("quadform")
    ks_ms, ks_n = eng.profile_read("kstar")
    sc_ms, sc_n = eng.profile_read("score")
    fu_ms, fu_n = eng.profile_read("fused_score")
    eng.profile(False)
    # the other leg (every rank scoring --candidates rows of its own), same protocol, for the side key
    other_leg = None
    if world > 1:
        if scaling == "strong":
            Xo = eng.dev(np.random.default_rng(101 + rank).random((M_arg, D)))
            o_lo, o_total, o_name = rank * M_arg, M_arg * world, "weak"
        else:
            lo_s, hi_s = shard_bounds(M_arg, rank, world)
            Xo = eng.dev(np.random.default_rng(1).random((M_arg, D))[lo_s:hi_s])
            o_lo, o_total, o_name = lo_s, M_arg, "strong"
        other = ShardedSearch(eng, post, Xo, o_lo, SCORE_POINTWISE_EI, mustar, collective="torch",
                              host_collective=share_gpu)
        o_elapsed, _ = timed_steps(other, args.steps)
        other_leg = {"scaling": o_name, "value": o_total * args.steps / o_elapsed, "unit": "evals/s",
                     "ms_per_step": o_elapsed / args.steps * 1e3, "M_total": o_total, "M_per_gpu": int(Xo.shape[0])}
        del Xo, other
    # the collective alone (rank 0 reports): the record is already on the device, so this is all-gather + reduction +
    # 16-byte read-back + the host's wait, i.e. the fixed cost a step pays on top of its kernels
    coll_us = None
    if use_dist and not share_gpu:
        rec = eng.predict_record(post, Xc[:256], SCORE_POINTWISE_EI, mustar, row_lo)
        gath = eng.empty(2 * world)
        for _ in range(5):
            dist.all_gather_into_tensor(gath, rec)
            eng.argmax_combine(gath)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(200):
            dist.all_gather_into_tensor(gath, rec)
            eng.argmax_combine(gath)
        torch.cuda.synchronize()
        coll_us = (time.perf_counter() - t0) / 200 * 1e6

    # ---- secondary rows of SURVEY 8d (rank 0 only, outside the timed region) ------------
    secondary = {}
    if rank == 0 and not args.no_secondary:
        def timed(fn, reps):
            fn()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t1) / reps
        F, W, b = F_RFF, W_rff, b_rff
        om = eng.dev(np.random.default_rng(5).standard_normal(F))
        t_proj = timed(lambda: eng.rff_project(Xd, W, b, th[2]), 10)
        eng.profile(True)
        t_rs = timed(lambda: eng.rff_score(Xc, W, b, th[2], om, want_score=False), 5)
        rs_ms, rs_n = eng.profile_read("rff_score")
        # K9: S, S_grad, diag(S_hessian) of the weight-space posterior from a resident Phi (random_fourier_sampler.py:106-122)
        Phi_res = eng.rff_project(Xd, W, b, th[2])
        t_terms = timed(lambda: eng.rff_terms(Phi_res, om, m, th[0]), 10)
        del Phi_res
        B, G, S = 512, 70, 150
        rngl = np.random.default_rng(6)
        al = np.linspace(0.005, 0.995, G)
        xs = rngl.random((B, D))
        dsel = np.arange(B) % D
        z = eng.dev(rngl.standard_normal((S, G)))
        xi_l, x_l = np.eye(D)[dsel], xs.copy()
        x_l[np.arange(B), dsel] = 0.0
        xi_d, x_d, al_d = eng.dev(xi_l), eng.dev(x_l), eng.dev(al)
        line_fn = lambda: eng.line_acq_xi(post, xi_d, x_d, al_d, z, mustar, jitter=1e-10 * float(th[2]) ** 2)
        t_line = timed(line_fn, 3)
        eng.profile(True)
        for _ in range(3):
            line_fn()
        torch.cuda.synchronize()
        lk = {k: eng.profile_read(k) for k in ("line_kstar", "line_y", "line_cov", "line_mc")}
        eng.profile(False)
        Ml = B * G
        mb = m + 1
        # executed MFMA flops: Y = G K*, every wavefront (32 rows of a 128-row tile) cut at the end of its last star (the
        # GEMM's per-wavefront K limit, as in quadform_kernel), and the covariance's data term: (lower-triangle tiles of
        # the ceil(G/16)^2 grid) x 2 products x N rows
        y_flops = sum(2.0 * 32 * Ml * min(N, -(-((bw + 1) * 32) // mb) * mb) for bw in range(-(-N // 32)))
        nt16 = -(-G // 16)
        cov_tiles = nt16 * (nt16 + 1) // 2 if (mb == 32) else nt16 * nt16
        cov_flops = 2.0 * B * cov_tiles * 2 * 256 * N
        line_ms = {k: v[0] / max(v[1], 1) for k, v in lk.items()}
        phi_bytes = 8.0 * F * N
        secondary = {
            "gram_kernel_larger_N": gram_sizes,
            "rff_project": {"F": F, "wall_ms_per_call": t_proj * 1e3, "avg_ms": pj_burst_ms, "bytes": phi_bytes,
                            "bound": "hbm", "achieved_GBs": phi_bytes / (pj_burst_ms * 1e-3) / 1e9,
                            "frac": phi_bytes / (pj_burst_ms * 1e-3) / 1e9 / PEAK_HBM_GBS,
                            "note": "avg_ms = steady state (HIP-graph replay of 100 launches); wall = one call incl. allocation "
                                    "and host launch latency"},
            "rff_score_evals_per_s": M / t_rs, "rff_score_kernel_ms": rs_ms / max(rs_n, 1),
            "rff_terms_ms": {"F": F, "N": N, "wall_ms_per_call": t_terms * 1e3,
                             "note": "S + S_grad + diag(S_hessian) in one call (reads Phi twice: 2 x 8 F N bytes); the reference: "
                                     "0.02 + 0.11 + 1.0 s"},
            "line_acq": {"lines": B, "grid": G, "draws": S, "ms": t_line * 1e3, "lines_per_s": B / t_line,
                         "entry": "ppbo_line_acq_xi (grid points formed on the device)",
                         "kernel_ms": {"kstar_kernel": line_ms["line_kstar"], "Y = G K* (dgemm_kernel, 128x128 tiles)": line_ms["line_y"],
                                       "line_cov_kernel": line_ms["line_cov"], "line_mc_kernel": line_ms["line_mc"]},
                         "bound": "mfma", "executed_flops": {"Y": y_flops, "covariance data term": cov_flops},
                         "achieved_TFLOPs_Y": y_flops / (line_ms["line_y"] * 1e-3) / 1e12,
                         "frac_Y": y_flops / (line_ms["line_y"] * 1e-3) / 1e12 / PEAK_FP64_MFMA_TFLOPS,
                         "achieved_TFLOPs_cov": cov_flops / (line_ms["line_cov"] * 1e-3) / 1e12,
                         "frac_cov": cov_flops / (line_ms["line_cov"] * 1e-3) / 1e12 / PEAK_FP64_MFMA_TFLOPS,
                         "frac": (y_flops + cov_flops) / (t_line) / 1e12 / PEAK_FP64_MFMA_TFLOPS,
                         "note": "frac = all executed MFMA flops of the call over its wall time (kstar, the Monte-Carlo part "
                                 "and launch gaps included) / fp64 MFMA peak"},
        }
        try:
            secondary["c1_loop"] = c1_loop(torch)
        except Exception as exc:          # noqa: BLE001
            secondary["c1_loop"] = {"error": repr(exc)}
        # the other BASELINE configurations on this GPU (the headline line is args.config): ~10 s in all
        for oc in ("c2", "c4", "c5"):
            if oc == args.config or args.no_other_configs:
                continue
            try:
                secondary[f"config_{oc}"] = other_config_row(torch, eng, oc)
            except Exception as exc:      # noqa: BLE001  -- a secondary row must never cost the headline line
                secondary[f"config_{oc}"] = {"error": repr(exc)}
        for pq_cfg in ("c2", "c3"):
            try:
                secondary[f"per_query_ms_{pq_cfg}"] = per_query_breakdown(torch, pq_cfg)
            except Exception as exc:      # noqa: BLE001  -- a secondary row must never cost the headline line
                secondary[f"per_query_ms_{pq_cfg}"] = {"error": repr(exc)}

    if rank == 0:
        ms_per_step = elapsed / args.steps * 1e3
        value = M_total * args.steps / elapsed
        # models of up to ~1024 rows are scored by ONE launch (csrc/fused.hip: K* in LDS, contraction, score); the
        # dominant kernel is then that launch, priced on the contraction's executed MFMA flops over its WHOLE duration
        fused_path = fu_n > 0 and qf_n == 0
        qf_avg_ms = (fu_ms / max(fu_n, 1)) if fused_path else qf_ms / max(qf_n, 1)
        qf_launches = fu_n if fused_path else qf_n
        mblk = m + 1
        # algorithmic flops of the variance contraction per launch: 2 M N^2 (dense A);
        # executed: the block-triangular G form does M * sum_tiles 2*128*kend(tile) flops
        # one launch scores a chunk of <= 65536 candidates (ppbo_predict's chunk_cap); the average is over launches
        M_launch = float(M) if fused_path else float(M) / max(1, -(-M // 65536))
        algo_flops = 2.0 * M_launch * N * N
        # executed: each wavefront owns 32 rows of a 128-row tile and stops at the end of their last star block
        # (equals SQ_INSTS_MFMA x 2048 of the rocprofv3 --pmc pass, profiles/)
        wrows = 32
        exec_flops = sum(2.0 * wrows * M_launch * min(N, -(-((b + 1) * wrows) // mblk) * mblk) for b in range(-(-N // wrows)))
        dense_equiv = algo_flops / (qf_avg_ms * 1e-3) / 1e12
        executed = exec_flops / (qf_avg_ms * 1e-3) / 1e12
        line = {
            "metric": "acquisition evals/sec (posterior mean + variance + EI + argmax per candidate)",
            "value": value, "unit": "evals/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": scaling, "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "config": {"workload": f"{wl_name}: N={N} obs rows (m={m}), D={D}, M={M_total} candidates in total "
                                   f"({M} on rank 0), {kern} theta={list(map(float, th))}", "name": args.config,
                       "N": N, "D": D, "M_total": M_total, "M_per_gpu": M,
                       "parallelism": f"candidates sharded x{world} ({scaling} scaling: M_total fixed at {M_total})"
                                      if scaling == "strong" else
                                      f"candidates sharded x{world} (weak scaling: {M} per GPU)",
                       "model_state": "replicated (every rank runs the same deterministic fit)",
                       "collective": ("none (single process)" if not use_dist else
                                      "gloo on host records [TEST MODE: ranks share one GPU]" if share_gpu else
                                      "1 all-gather of a 16-byte device record per step, " +
                                      ("torch.distributed nccl (RCCL) + ppbo_argmax_combine" if args.collective == "torch"
                                       else "the library's own RCCL communicator (ppbo_search_sharded)"))},
            "ms_per_step_with_event_brackets": elapsed_bracketed / args.steps * 1e3,
            "collective_roundtrip_us": coll_us,
            "gp_fit_ms": gp_fit_ms, "gp_fit_ms_runs": fit_runs, "gp_fit_ms_min": min(fit_runs),
            "gp_fit_ms_from_f_init": gp_fit_ms_from_f_init, "gp_fit_ms_from_f_init_runs": fit_runs_f,
            "gp_fit_ms_protocol": "median of %d timed runs after one warm-up; gp_fit_ms: start handed over as z0 = L^-1 f_init "
                                  "(what the drop-in does: it draws z0 itself); gp_fit_ms_from_f_init: the stored f_init itself, "
                                  "nothing precomputed outside the timed call (%d L-BFGS evaluations)" % (n_fit, st_f["lbfgs_evals"]),
            "gp_fit_start": fit_start, "gp_fit_iterations": st["iterations"],
            "gp_fit_cholesky": st["n_cholesky"],
            "replicated_fit_bitwise_equal": replicated_equal,
            "gp_fit_method": "ppbo_gp_fit: one call = Gram, Cholesky, [triangular inverse, Sigma^-1 on a second stream beside the first evaluations], whitened L-BFGS (z = L^-1 f; "
                             "trust-region finisher only if it does not end on |grad_f T| < gtol), posterior",
            "gp_fit_lbfgs": {"iterations": st["lbfgs_iterations"], "evals": st["lbfgs_evals"], "status": st["lbfgs_status"]},
            "gp_fit_trust_region_only": None if tr_st is None else {
                "ms": tr_fit_ms, "iterations": tr_st["iterations"], "cholesky": tr_st["n_cholesky"]},
            "gp_fit_breakdown": {"potrf_calls": potrf_n, "potrf_avg_ms": potrf_ms / max(potrf_n, 1),
                                 "potrf_total_ms": potrf_ms,
                                 "note": "factorizations incl. Sigma^-1 and the posterior; failed ones end early"},
            # achieved / frac = MFMA flops the kernel EXECUTES (block-triangular G) over the live event
            # time: never above 1.  The dense-A figure SURVEY 8(d) prices (2 M N^2) is the side key.
            "roofline": {"bound": "mfma",
                         "kernel": ("fused_score_kernel (K2+K3+K4 in one launch: K* in LDS, |G K*|^2, score; flops = the "
                                    "contraction's, time = the whole launch)") if fused_path else "quadform_kernel (K4: |G K*|^2)",
                         "achieved": executed,
                         "peak": PEAK_FP64_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": executed / PEAK_FP64_MFMA_TFLOPS,
                         "traffic": None, "avg_launch_ms": qf_avg_ms, "launches": qf_launches,
                         "executed_flops_per_launch": exec_flops,
                         "dense_equivalent_flops_per_launch": algo_flops, "dense_equivalent_tflops": dense_equiv},
            "kernels": {
                "kstar_kernel": {"avg_ms": ks_ms / max(ks_n, 1), "launches": ks_n},
                "score_kernel": {"avg_ms": sc_ms / max(sc_n, 1), "launches": sc_n},
                "gram_kernel": dict(gram_c3 or {}, bound="hbm", peak_GBs=PEAK_HBM_GBS,
                                    avg_ms=(gram_c3 or {}).get("streaming_ms"),
                                    note="steady state: HIP-graph replay of 100 launches, clocks settled under the kernel's "
                                         "own load.  `frac` = streaming rate (outputs rotated over > 512 MB, every byte reaches "
                                         "HBM) / 8 TB/s; `resident_*` = one output buffer, which at this N sits in the 256 MB "
                                         "Infinity Cache (a fabric / L3 write rate, not an HBM rate); `write_only_floor_*` = "
                                         "ppbo_store_floor measured in this run over the same rotating buffers"),
            },
            "secondary": secondary,
            "best": {"value": best[0], "index": best[1]},
            ("weak_scaling_leg" if scaling == "strong" else "strong_scaling_leg"): other_leg,
        }
        # `traffic` = HBM-side (fabric) bytes per launch of the dominant kernel from the PMC counters.  rocprofv3 --pmc passes
        # cannot run inside this process: the number comes from the last committed capture (profiles/r0*_pmc_hot_kernels.json:
        # FETCH_SIZE x 2 -- the gfx950 correction of /opt/skills/guides/MI355X_MICROARCH.md -- + WRITE_SIZE), and ONLY while
        # it belongs to this launch shape; `traffic_source.current` says whether the kernel sources are still the ones it
        # was taken with (tools/pmc_quadform.sh / tools/dev/r6_fused_pmc.sh record the csrc digest).  `algorithmic_bytes` is
        # what the launch must move: three-launch form = K* once + G's block triangle + the slab written; one-launch form
        # = candidates + G's block triangle once per 32 candidates' workgroup (L2 traffic, not HBM: G is L2-resident) --
        # there the HBM-side figure is the candidates, X and G once.
        import glob
        pmcs = sorted(glob.glob(os.path.join(ROOT, "profiles", "r0*_pmc_hot_kernels.json")))
        pmc = pmcs[-1] if pmcs else ""
        tri = sum(8.0 * wrows * min(N, -(-((b + 1) * wrows) // mblk) * mblk) for b in range(-(-N // wrows)))   # G's block triangle
        if fused_path:
            line["roofline"]["algorithmic_bytes"] = 8.0 * (M_launch * D + N * D + 3 * N) + tri + 16.0 * (M_launch / 32)
        else:
            line["roofline"]["algorithmic_bytes"] = 8.0 * N * M_launch + tri + 8.0 * (-(-N // 128)) * M_launch
        if pmc and os.path.exists(pmc):
            try:
                from ppbo_amd.build import _digest
                doc = json.load(open(pmc))
                key = "fused_score" if fused_path else "quadform"
                ent = doc.get(key) or {}
                d = ent.get("derived") or {}
                shape_ok = ent.get("shape", {"N": 2048, "M": 65536}) == {"N": N, "M": int(M_launch)}
                if d and shape_ok:
                    line["roofline"]["traffic"] = d["fabric_read_bytes(FETCH_SIZE KB x1024 x2 gfx950 correction)"] + d["write_bytes"]
                    line["roofline"]["traffic_over_algorithmic"] = line["roofline"]["traffic"] / line["roofline"]["algorithmic_bytes"]
                line["roofline"]["traffic_source"] = {
                    "file": f"profiles/{os.path.basename(pmc)}", "entry": key, "shape_matches_this_launch": bool(d and shape_ok),
                    "counters": "FETCH_SIZE x 2 (gfx950 correction) + WRITE_SIZE, separate --pmc passes, per launch",
                    "csrc_digest": doc.get("csrc_digest"), "current": doc.get("csrc_digest") == _digest()}
                # (the key earlier rounds printed; kept so that old and new lines compare)
                if d:
                    line["roofline"]["traffic_from_profile"] = {
                        "bytes_per_launch": d["fabric_read_bytes(FETCH_SIZE KB x1024 x2 gfx950 correction)"] + d["write_bytes"],
                        "source": f"profiles/{os.path.basename(pmc)} ({key})",
                        "csrc_digest": doc.get("csrc_digest"), "current": doc.get("csrc_digest") == _digest()}
            except Exception:
                pass
        # model on the REFERENCE's f_MAP (fixture): parity of the timed path on the fixture's candidates, and
        # BASELINE config 5's "fp32 tolerance check": the same scoring with K* evaluated in fp32 (fp64 accumulation)
        need_ref = (not args.no_precision_report) or (world == 1 and not args.no_cpu_baseline and args.config in ("c2", "c3"))
        if need_ref:
            Sinv_d = eng.pd_inverse(eng.gram(Xd, th, kern))
            post_ref = eng.posterior(Xd, th, kern, Sinv_d, g["fMAP"], m)
        sf2 = float(th[2]) ** 2
        rep = {}
        for nm, f32 in (() if args.no_precision_report else (("fp64", False), ("fp32_kstar", True))):
            o = eng.predict(post_ref, g["Xc"], want_best=False, kstar_fp32=f32)
            rep[nm] = {"mu_max_rel_err": float(np.abs(o["mu"].cpu().numpy() - g["mu"]).max() / np.abs(g["mu"]).max()),
                       "var_max_err_over_sf2": float(np.abs(o["var"].cpu().numpy() - g["var"]).max() / sf2)}
        if rep:
            rep["note"] = ("errors against the reference's own mu / diag Sigma_pred on the fixture's 512 candidates; tolerance 1e-5 "
                           "applies to fp64 (the product path); the fp32-K* variant is reported, not shipped")
            line["secondary"]["precision_report"] = rep
        if world == 1 and not args.no_cpu_baseline and args.config in ("c2", "c3"):   # sigma = 0.001 oracle fits (c4, c5) take minutes to hours
            # the oracle uses the reference's fMAP from the fixture; score the same subsample with that model
            Xs = np.random.default_rng(11).random((256, D))
            chk = eng.predict(post_ref, Xs, want_best=False)
            line["cpu_baseline"] = cpu_baseline(g, 2048, gpu_check=(Xs, chk["mu"].cpu().numpy(), chk["var"].cpu().numpy()))
        if args.dump_outputs:
            # the record the last timed step returned (ShardedSearch.step: best score, global row index), identical on every
            # rank; the index is exact in float64
            os.makedirs(args.dump_outputs, exist_ok=True)
            np.save(os.path.join(args.dump_outputs, "best_score.npy"), np.array([best[0]], dtype=np.float64))
            np.save(os.path.join(args.dump_outputs, "best_index.npy"), np.array([best[1]], dtype=np.float64))
        print(json.dumps(line))
    search.close()
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
