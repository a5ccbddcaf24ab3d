"""The small-mean Poisson increments of rip_synth_apportion (synth.hip) on the device, measured:

  census   for the library in use: 4096 pixels x 36 reads per mean of tests/synth_deviates_cases.SMALL_MEANS -- draws, the share
           the reference pins, draws outside their interval, draws that left the plain f64 quantile ppf(u) and the largest
           |u - nearest cdf step| among those; then every listed extreme-bin seed over the grid of means: device count against
           ppf(u) and the interval
  timing   rip_synth_apportion alone at 4096 x 4096 pixels, 35 reads, 4.7 electrons per read (the sky's straight-line code:
           2.8 ms by the kernel's own note), 10 calls after 3 of warm-up between two host time stamps around a synchronised
           stream; with --ab LIB each round runs LIB (ROMANHIP_LIB) and the library in the tree in fresh processes, alternating

  python tools/gpu_checks/synth_deviates.py census
  python tools/gpu_checks/synth_deviates.py timing [--ab other/libromanhip.so] [--rounds 5]
"""
import argparse
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import numpy as np  # noqa: E402


def apportion_ms():
    import torch  # noqa: F401  (before the library: one HIP runtime for both)

    from romanimpreprocess_amd import _native

    ctx = _native.default_context(0)
    dev = torch.device("cuda", 0)
    n, nreads = 4096, 35
    c = torch.full((n, n), 4.7 * nreads, dtype=torch.float32, device=dev)
    out = torch.empty((nreads, n, n), dtype=torch.int32, device=dev)
    t = np.arange(1, nreads + 1, dtype=np.float64)
    torch.cuda.synchronize()
    for _ in range(3):
        ctx.call("rip_synth_apportion", c, n, n, True, nreads, t, 7, out)
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
        ctx.call("rip_synth_apportion", c, n, n, True, nreads, t, 7, out)
    ctx.synchronize()
    return (time.perf_counter() - t0) * 100.0


def timing(ab, rounds):
    if ab is None:
        print("%.4f" % apportion_ms())
        return 0
    libs = (("other", os.path.abspath(ab)), ("tree", None))
    ms = {name: [] for name, _ in libs}
    for r in range(rounds):
        for name, path in libs:
            env = dict(os.environ)
            env.pop("ROMANHIP_LIB", None)
            if path:
                env["ROMANHIP_LIB"] = path
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "timing"], env=env, capture_output=True, text=True, timeout=120)
            if res.returncode != 0:
                print(res.stdout, res.stderr)
                return res.returncode     # nothing more is started on the GPU
            ms[name].append(float(res.stdout.split()[-1]))
            print("round %d %-5s %.4f ms per frame" % (r, name, ms[name][-1]), flush=True)
    for name, path in libs:
        v = np.array(ms[name])
        print("%-5s (%s): median %.4f ms, range %.4f .. %.4f (%.4f), %d rounds of 10 calls" %
              (name, path or "the tree's library", np.median(v), v.min(), v.max(), v.max() - v.min(), len(v)))
    return 0


def census():
    import torch  # noqa: F401
    from scipy import special

    import synth_deviates_cases as cases
    import synth_deviates_ref as ref
    from romanimpreprocess_amd import _native

    ctx = _native.default_context(0)
    dev = torch.device("cuda", 0)

    def apportion(counts, t, seed):
        c = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.float32)).to(dev)
        out = torch.full((len(t), c.numel()), -77, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ctx.call("rip_synth_apportion", c, 1, c.numel(), True, len(t), t, seed, out)
        ctx.synchronize()
        return out.cpu().numpy().astype(np.float64)

    print("library:", _native.LIB_PATH)
    npix, nreads = 4096, 36
    t = np.arange(1, nreads + 1, dtype=np.float64)
    ks = np.arange(0, 200, dtype=np.float64)
    for mean in cases.SMALL_MEANS:
        counts = np.full(npix, mean * nreads, dtype=np.float32)
        f = ref.PoissonFrame(counts, t, 0xCE5505)
        d = np.diff(apportion(counts, t, 0xCE5505), axis=0, prepend=0.0)
        plain = ref.poisson_ppf(f.u, f.lam)
        outside = (d < f.lo) | (d > f.hi)
        left = d != plain
        steps = special.pdtr(ks, float(f.lam[0, 0]))
        dist = np.min(np.abs(f.u[left][:, None] - steps[None, :]), axis=1) if left.any() else np.zeros(1)
        print("mean %-5g: %d draws, pinned %.4f %%, outside their interval %d, off ppf(u) %d, largest |u - cdf step| among those %.3g (%.2f x 2^-24)"
              % (mean, d.size, 100.0 * f.pinned.mean(), outside.sum(), left.sum(), dist.max(), dist.max() * 2.0 ** 24))
    means = np.array(cases.EXTREME_MEANS)
    for seed, npx, nrd, pixel, read, value in cases.EXTREME_BINS:
        tt = np.arange(1, nrd + 1, dtype=np.float64)
        u = float(ref.small_uniform(value))
        got = np.zeros(len(means))
        lam = np.zeros(len(means))
        for j, m in enumerate(means):
            counts = np.full(npx, m * nrd, dtype=np.float32)
            col = apportion(counts, tt, seed)[:, pixel]
            got[j] = col[read] - (col[read - 1] if read else 0.0)
            lam[j] = float(counts[0]) * (1.0 / nrd)
        lo, hi = ref.small_interval(np.full(len(means), u), lam)
        plain = ref.poisson_ppf(np.full(len(means), u), lam)
        bad = (got < lo) | (got > hi)
        worst = int(np.argmax(got - plain))
        print("seed %4d pixel %4d read %d bin %#08x: %3d of %d means outside, %3d off ppf(u); largest excess at mean %.4f: device %g, ppf(u) %g, "
              "interval %g .. %g" % (seed, pixel, read, value, bad.sum(), len(means), np.count_nonzero(got != plain), means[worst],
                                     got[worst], plain[worst], lo[worst], hi[worst]))
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("census", "timing"))
    ap.add_argument("--ab", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    sys.exit(census() if a.what == "census" else timing(a.ab, a.rounds))
