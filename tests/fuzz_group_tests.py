"""The seeded cases that tests/test_fuzz_group_tests_host.py and tests/test_gpu_fuzz_group_tests.py share: 40 draws of a
shape of st_group_sums_codes -- n in 3 .. 300, 1 .. 12 groups (some labels without an object), 0 .. 9 permutations, a
chunk, a slice length, full-range int32 codes."""
import numpy as np

N_CASES = 40


def case(k):
    """{y, group, n_groups, permutations, seed, stream, chunk_tasks, slice} of case k"""
    rng = np.random.default_rng(27000 + k)
    n = int(rng.integers(3, 301)) if k >= 4 else (3, 4, 5, 300)[k]
    n_groups = int(rng.integers(1, 13))
    wide = rng.integers(0, 2)
    y = rng.integers(-(1 << 31), 1 << 31, n * (n - 1) // 2, dtype=np.int64) if wide else rng.integers(-3, 4, n * (n - 1) // 2)
    return dict(y=y.astype(np.int32), group=rng.integers(0, n_groups, n).astype(np.uint8), n_groups=n_groups,
                permutations=int(rng.integers(0, 10)), seed=int(rng.integers(0, 1 << 63)), stream=int(rng.integers(0, 1000)),
                chunk_tasks=int(rng.choice([0, 1, 2, 5, 40, 1000])), slice=int(rng.choice([1, 2, 3, 4, 5, 16, 64, 256])))


def run(c, device, monkeypatch, plain=False):
    """the sums of case c on ``device``; ``plain``: without its chunk and slice"""
    from suchtree_amd import _capi
    if plain:
        monkeypatch.delenv("SUCHTREE_AMD_GROUP_SLICE", raising=False)
    else:
        monkeypatch.setenv("SUCHTREE_AMD_GROUP_SLICE", str(c["slice"]))
    return _capi.group_sums_codes(c["y"], c["group"], c["n_groups"], c["permutations"], c["seed"], c["stream"], device,
                                  0 if plain else c["chunk_tasks"])
