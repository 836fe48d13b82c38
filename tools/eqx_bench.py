#!/usr/bin/env python3
"""What --eqx (MM_F_EQX) costs a mapping run, with the =/X CIGARs written on the device (cigar_eqx_kernel) and with the host's route.

    python tools/eqx_bench.py [--ref-mb 200] [--gbases 6.0] [--repeat 2] [--threads 16] [--workloads map-hifi,map-ont] [--out profiles/eqx_bench.json]

Per workload -- map-hifi (~15 kb reads, 0.5 % error) and map-ont (~10 kb, 12 %) on one synthetic reference, reads made by bench.py's generators --
three rows, one Aligner each, mapping only (mm_gpu_map_staged around a staged batch; no text is written):
  plain       without --eqx;
  eqx         --eqx, the device route: the reads stay on the chains -> hits -> windows -> consume -> finish path, cigar_eqx_kernel on top;
  eqx_host    --eqx with MM2AMD_DEVICE_EQX=0: the host's plan / consume rounds and the host's mm_update_cigar_eqx.
A row maps the batch once to warm up, --repeat times with the profiler off for the rate and the process's CPU seconds, once more with the profiler
on for the kernels' milliseconds.  One JSON object, printed and written to --out."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"map-hifi": (15000, 0.005), "map-ont": (10000, 0.12)}
ROWS = [("plain", False, None), ("eqx", True, None), ("eqx_host", True, "0")]


def kernel_ms(prof, prefix):
    return sum(v["ms"] for k, v in prof.items() if k.startswith(prefix))


def main(argv=None):
    import torch
    import bench
    import minimap2_amd as mm
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-mb", type=float, default=200.0)
    ap.add_argument("--gbases", type=float, default=6.0)
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--workloads", default="map-hifi,map-ont")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eqx_bench.json"))
    a = ap.parse_args(argv)
    L = mm.lib()
    if L.mm2amd_device_count() < 1:
        raise SystemExit("eqx_bench needs a GPU: " + L.mm2amd_last_error().decode())
    dev = torch.device("cuda", 0)
    res = {"backend": L.mm2amd_backend_name().decode(), "ref_mb": a.ref_mb, "repeat": a.repeat, "threads": a.threads, "workloads": {}}
    try:
        res["commit"] = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:  # noqa: BLE001
        res["commit"] = None
    total = int(a.ref_mb * 1e6)
    n_contig = max(1, min(24, total // 1000000))
    codes, per = bench.gen_reference(torch, dev, 11, total, n_contig)
    refs = bench.reference_ascii(torch, dev, codes, per, n_contig)
    names = ["chr%d" % (i + 1) for i in range(n_contig)]
    for preset in a.workloads.split(","):
        mean_len, err = WORKLOADS[preset]
        n_reads = max(1, int(a.gbases * 1e9 / mean_len))
        reads, chunk = [], max(1, min(n_reads, int(1.0e9 // mean_len)))
        for c0 in range(0, n_reads, chunk):
            reads += bench.gen_reads(torch, dev, 1000 + 7919 * (c0 // chunk), codes, per, n_contig, min(chunk, n_reads - c0), mean_len, mean_len // 10, err)
            torch.cuda.empty_cache()
        bases = float(sum(len(r) for r in reads))
        batch = mm.Batch([("read%d" % i, s) for i, s in enumerate(reads)])
        rows = {}
        for name, eqx, env in ROWS:
            os.environ.pop("MM2AMD_DEVICE_EQX", None)
            if env is not None:
                os.environ["MM2AMD_DEVICE_EQX"] = env
            al = mm.Aligner(refs, preset=preset, names=names, n_threads=a.threads, sam=True, eqx=eqx)
            try:
                wall, cpu, st, prof = [], [], None, {}
                for it in range(a.repeat + 2):  # warm-up, the timed runs, one run for the kernels' events
                    profiled = it == a.repeat + 1
                    al.stage(batch)
                    if profiled:
                        mm.profile_enable(True)
                    t0, c0 = time.perf_counter(), time.process_time()
                    n_reg, reg, _ = al.run(raw=True)
                    t1, c1 = time.perf_counter(), time.process_time()
                    if profiled:
                        prof = mm.profile_get()
                        mm.profile_enable(False)
                    elif it:
                        wall.append(t1 - t0), cpu.append(c1 - c0)
                    st = al.last_stats()
                    al.free_raw(n_reg, reg)
            finally:
                al.close()
                os.environ.pop("MM2AMD_DEVICE_EQX", None)
            rows[name] = {"gbases_per_s": [bases / w / 1e9 for w in wall], "host_core_seconds_per_gbase": [c / (bases / 1e9) for c in cpu], "wall_s": wall,
                          "n_region_reads_dev": int(st["n_region_reads_dev"]), "n_region_reads_host": int(st["n_region_reads_host"]),
                          "region_finish_kernel_ms": kernel_ms(prof, "region_finish_kernel"), "cigar_eqx_kernel_ms": kernel_ms(prof, "cigar_eqx_kernel"),
                          "cigar_eqx_kernel_rows": {k: v for k, v in prof.items() if k.startswith("cigar_eqx_kernel")}}
            print("[eqx_bench] %s %s: %.3f Gbases/s, %.2f host core-s/Gbase, %d reads on the device route, finish %.1f ms, eqx %.1f ms" % (
                preset, name, max(rows[name]["gbases_per_s"]), min(rows[name]["host_core_seconds_per_gbase"]), rows[name]["n_region_reads_dev"],
                rows[name]["region_finish_kernel_ms"], rows[name]["cigar_eqx_kernel_ms"]), file=sys.stderr, flush=True)
        res["workloads"][preset] = {"reads": len(reads), "bases": bases, "mean_len": mean_len, "err": err, "rows": rows,
                                    "eqx_over_eqx_host": max(rows["eqx"]["gbases_per_s"]) / max(rows["eqx_host"]["gbases_per_s"]),
                                    "eqx_over_plain": max(rows["eqx"]["gbases_per_s"]) / max(rows["plain"]["gbases_per_s"])}
        del reads, batch
    line = json.dumps(res, sort_keys=True)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(res, sort_keys=True, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
