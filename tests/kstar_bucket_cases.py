"""The case matrix of tests/test_gpu_kstar_buckets.py: every radial family in every padded-dimension bucket of the K*
launchers of ppbo_amd/csrc/predict.hip, at both edges of the bucket.  Pure Python (no torch, no GPU):
tests/test_kstar_bucket_cases_host.py ties it to the launch ladders in the source.

One case per (bucket b, family k), 44 in all:
  * D is the bucket's upper edge BUCKETS[b] (no padded column) when b + k is even, else its lower edge BUCKETS[b - 1] + 1
    (the most padded columns).  The bucket 4 takes D = 2 as its lower edge: at D = 1 every star of the design lies on one
    line, and D = 1 is run by tests/test_gpu_gradients.py and test_gpu_parity.py::test_every_dimension_bucket;
  * the variance operator's form is node when b + k // 2 is even, else edge;
  * the design is (n_q, m) = (8, 3), N = 32, when b is even, else (3, 25), N = 78: off every tile edge, and a star of 26
    rows spans two KS_RJ = 32 staging steps of the K* kernels.
So every (family, DP) instance of every launcher runs once, and every bucket sees both edges in both forms.  The lower
edges of the coarser ladders (kstar_func_kernel's 8 / 20 / 32 / 48 / 64 and the fp32 report's 6 / 20 / 64) are lower edges
of this one: 2, 9, 21, 33, 49 and 2, 7, 21."""
from collections import namedtuple

BUCKETS = (4, 6, 8, 10, 12, 16, 20, 24, 32, 48, 64)
FAMILIES = ("SE_kernel", "RQ_kernel", "Matern52_kernel", "Matern32_kernel")
SHAPES = ((8, 3), (3, 25))              # (n_q, m) of an even / an odd bucket index
# the launchers of predict.hip that this matrix is run through, and the entry point that reaches each
LAUNCHERS = {
    "launch_kstar": "predict (PPBO_FUSED=0; kstar_fp32; the pruned search's flagged instance)",
    "launch_kstar_pair": "predict_pairs",
    "launch_kstar_slope": "predict_slopes",
    "launch_kstar_grad": "predict_gradients",
    "launch_kstar_curv": "predict_curvatures (with accelerations for D <= 16)",
    "launch_kstar_func": "predict_functionals",
}

Case = namedtuple("Case", "b k kernel D edge form n_q m")


def lower_edge(ladder, n):
    """The smallest D that the rung n of a ladder (the sorted DP values of one if-chain) serves; 2 in the first rung."""
    ladder = sorted(ladder)
    i = ladder.index(n)
    return 2 if i == 0 else ladder[i - 1] + 1


def case(b, k):
    upper = (b + k) % 2 == 0
    n_q, m = SHAPES[b % 2]
    return Case(b=b, k=k, kernel=FAMILIES[k], D=BUCKETS[b] if upper else lower_edge(BUCKETS, BUCKETS[b]),
                edge="upper" if upper else "lower", form="node" if (b + k // 2) % 2 == 0 else "edge", n_q=n_q, m=m)


def case_id(c):
    return f"{c.kernel[:-7]}-D{c.D}-{c.form}"


CASES = tuple(case(b, k) for b in range(len(BUCKETS)) for k in range(len(FAMILIES)))
