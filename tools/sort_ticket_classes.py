"""GPU box, trace build of the tile sort (tools/build_variant_all.sh sorttrace -DGSR_TRACE_SORT; GSR_HIP_LIB=.../libgsr_sorttrace.so):
where a tile_sort launch's time goes, per list-length class.  The scene and the step are bench.py's (100 k Gaussians, 800 x 800, V ring
cameras, forward + backward): V=4 is `bench.py --config 3`, V=1 / V=8 are `--views 1` / `--views 8`.

    python tools/sort_ticket_classes.py 4 1 8

Per class: tickets, who sorts them (w = one wave, ww = a pair of waves, W = a 4-wave workgroup), median and longest duration, the moment the class's last
ticket ends; then the launch's total, the moment the last workgroup entered the kernel, and the work = sum over all tickets of
duration x waves, divided by the wave slots of the chip (CUs x 4 SIMDs x the kernel's waves per SIMD).  Times in us since the first
workgroup entered the kernel (wall_clock64, 10 ns steps).  A ticket's end is taken when its stores are ISSUED."""
import ctypes as C, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gs-dynamics_amd")):
    sys.path.insert(0, p)
from diff_gaussian_rasterization import _hip
from gsdyn import synth_ring_cameras, synth_scene_params
from gsdyn.step import render_step_views

CLASSES = (64, 128, 256, 512, 1016)
WAVES_PER_SIMD = int(os.environ.get("TS_MIN_WAVES", "7"))
N = 65536


def trace(lib, V, dev):
    params = synth_scene_params(100_000, seed=0, device=dev)
    cams = synth_ring_cameras(V, 800, 800, device=dev)
    dL = torch.tensor(np.random.default_rng(1234).uniform(-1, 1, (V, 3, 800, 800)).astype(np.float32), device=dev)
    for _ in range(5):
        render_step_views(params, cams, dL)
    torch.cuda.synchronize()
    buf, wg = (C.c_uint32 * (4 * N))(), (C.c_uint32 * N)()
    assert lib.gsr_debug_sort_trace(buf, wg, N) == 0
    a = np.frombuffer(buf, dtype=np.uint32).reshape(N, 4).astype(np.int64)
    n_wg = V * ((800 + 15) // 16) ** 2
    return a[a[:, 3] > 0], np.frombuffer(wg, dtype=np.uint32).astype(np.int64)[:n_wg]


def table(V, a, wg_start):
    # the arrays keep older calls' tickets at ids this launch did not write (warm-up calls of the same shape overwrite them all; a
    # stale record shows as a start far from the rest)
    base = wg_start.min()
    a = a[(a[:, 0] >= base) & (a[:, 0] - base < 100_000)]
    t0, t1, kind, ln = (a[:, 0] - base) / 100.0, (a[:, 1] - base) / 100.0, a[:, 2] >> 24, a[:, 3]
    dur, waves = t1 - t0, np.where(kind == 1, 4, np.where(kind == 2, 2, 1))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    slots = cus * 4 * WAVES_PER_SIMD
    print(f"views {V}: {len(a)} tickets, {len(wg_start)} workgroups, {int(ln.sum())} entries, longest list {int(ln.max())}")
    print(f"  {'class':>10} {'tickets':>8} {'by':>3} {'median us':>10} {'longest us':>11} {'last start us':>14} {'last end us':>12}")
    lo = 0
    for hi in CLASSES + (1 << 30,):
        m = (ln > lo) & (ln <= hi)
        if m.any():
            by = "".join(sorted({{1: "W", 2: "ww"}.get(int(k), "w") for k in np.unique(kind[m])}))
            name = f"<= {hi}" if hi < (1 << 30) else "> 1016"
            print(f"  {name:>10} {int(m.sum()):8d} {by:>3} {np.median(dur[m]):10.2f} {dur[m].max():11.2f} {t0[m].max():14.2f} {t1[m].max():12.2f}")
        lo = hi
    last = int(np.argmax(t1))
    print(f"  launch: last ticket ends at {t1.max():.2f} us (a list of {int(ln[last])} entries, started at {t0[last]:.2f});"
          f" last workgroup entered at {(wg_start.max() - base) / 100.0:.2f} us")
    print(f"  work: sum of duration x waves = {(dur * waves).sum():.0f} wave-us; / {slots} wave slots = {(dur * waves).sum() / slots:.2f} us")
    edges = np.arange(0.0, t1.max() + 2.0, 2.0)
    print("  window us: waves busy (avg), tickets ending")
    for e in edges[:-1]:
        ov = (np.clip(np.minimum(t1, e + 2) - np.maximum(t0, e), 0, None) * waves).sum() / 2.0
        print(f"    {e:5.0f}-{e + 2:<5.0f} {ov:8.0f} {int(((t1 >= e) & (t1 < e + 2)).sum()):6d}")


if __name__ == "__main__":
    dev = torch.device("cuda:0")
    lib = _hip.load_library()
    lib.gsr_debug_sort_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    for v in [int(x) for x in sys.argv[1:]] or [4]:
        table(v, *trace(lib, v, dev))
