#!/usr/bin/env python
"""Seconds per call, and bytes per second, of the transposes of a batch's
device-resident boundary: get_state_device, set_state_device (all
environments, and a 10 % mask) and set_xfrc_device (its check and its
transpose), timed with device events on the batch's stream.

multi_sphere4 at E = 1,048,576 by default: 4 M rows, so that the caller's
arrays and the batch's rows each exceed the 256 MiB Infinity Cache.  Every
timing is `--calls` calls between two events after a warm-up, repeated
`--reps` times.  Bytes are what a call must move, from the shapes: per row

  get_state_device   13 reals read (x y z of the snapshot, 10 state rows), 13 elements written
  set_state_device   13 elements and the bounding radius read, the snapshot (4 reals) and 13 rows written
  set_xfrc_device    6 elements read twice (check, transpose), 6 reals written

(masked: that per row of a masked environment, and the mask).  The share is
of the 8.0 TB/s HBM3E peak of the MI355X.

Prints one JSON line and writes it to --out.  Needs the GPU.
"""
import argparse
import json
import os
import sys


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rigidbody-simulation_amd"))

HBM_PEAK = 8.0e12


def _summary(x):
    r = sorted(x)
    return dict(median=r[len(r) // 2], min=r[0], max=r[-1], reps=x)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--envs", type=int, default=1 << 20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch", "dev_transposes.json"))
    a = ap.parse_args()

    import torch
    import rbhip
    from rbhip import scenes
    rbhip.load()
    sc = scenes.multi_sphere4()
    E, M = a.envs, sc.n
    N = E * M
    real = 8 if a.dtype == "f64" else 4
    io = 8                                              # float64 tensors
    with rbhip.BatchWorld(sc, E, dtype=a.dtype) as b:
        b.use_stream(torch.cuda.current_stream().cuda_stream)
        dev = f"cuda:{b.device}"
        q, v = b.get_state_device(dtype="f64")
        xf = torch.zeros((E, M, 6), dtype=torch.float64, device=dev)
        mask = torch.zeros(E, dtype=torch.bool, device=dev)
        mask[::10] = True
        n_masked = int(mask.sum().item())
        cases = {
            "get_state_device": (lambda: b.get_state_device(q, v), N * 13 * (real + io)),
            "set_state_device": (lambda: b.set_state_device(q, v), N * (13 * io + real + 17 * real)),
            "set_state_device_mask10": (lambda: b.set_state_device(q, v, mask=mask),
                                        n_masked * M * (13 * io + real + 17 * real) + E),
            "set_xfrc_device": (lambda: b.set_xfrc_device(xf), N * 6 * (2 * io + real)),
        }
        times = {name: [] for name in cases}
        for name, (call, _) in cases.items():
            for _ in range(3):
                call()
            b.sync()
            for _ in range(a.reps):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.calls):
                    call()
                t1.record()
                t1.synchronize()
                times[name].append(t0.elapsed_time(t1) * 1e-3 / a.calls)
        b.sync()
    res = dict(bench="batch_dev_transposes", scene="multi_sphere4", envs=E, rows=N, dtype=a.dtype, io="f64",
               calls=a.calls, unit="seconds per call", hbm_peak_bytes_per_s=HBM_PEAK,
               version=rbhip.load().rb_version().decode(), cases={})
    for name, (_, nbytes) in cases.items():
        s = _summary(times[name])
        s.update(bytes=nbytes, bytes_per_s=nbytes / s["median"], share_of_hbm_peak=nbytes / s["median"] / HBM_PEAK)
        res["cases"][name] = s
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
