"""save_ply from device tensors (gsr_ply_save) against what a caller had to write
without it: upstream's GaussianModel.save_ply restated with torch `.cpu()`, numpy.concatenate and
a structured array's tofile -- on the same GPU, into the same directory, in the same process.

For every P (default 1M and 6M) at SH degree 3 (62 float32 columns, 248 bytes per row), serial,
after a warm-up, the two paths alternating:

  hip       save_ply(path, scene): k_ply_pack into two device slots, two pinned host slots, write().
  restated  six `.detach()...cpu().numpy()` copies (f_dc and f_rest through transpose(1, 2)
            .flatten(1).contiguous(), as upstream), zeros for the normals, numpy.concatenate to
            [P, 62], a structured array of 62 'f4' fields filled from it, the header plyfile writes
            and `tofile`.  This is kinder than upstream, whose `elements[:] = list(map(tuple,
            attributes))` builds P Python tuples and is not run at these sizes.

Reported per (P, path): call_s, a host clock around the whole call (both end synchronised, the file
complete and closed); file_gb_per_s = file bytes over it; peak_host_mb, the largest growth of the
process's resident set during a call, sampled every 2 ms from /proc/self/statm by a thread (pinned
staging is resident memory and counts).  The first pair of files is compared byte for byte.  The
directory is /dev/shm when it is there and has room for both files, else the working directory;
the result lines say which.  A file in /dev/shm is memory: the figures are the paths' own cost, not
a disk's.

The pack kernel alone comes from a kernel trace of a run of its own:

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o trace -- \\
      python tools/bench_ply_save.py --P 6000000 --paths hip
  python tools/bench_ply_save.py --kernel-stats DIR --P 6000000

prints k_ply_pack's calls and time per save and its rate against the byte floor 2 x 4R x P (every
source word read once, every file word written once).

Usage: python tools/bench_ply_save.py [--P 1000000 6000000] [--steps 3] [--warmup 1]
[--paths hip restated] [--dir DIR]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import sys
import threading
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

M = 16
R = 17 + 3 * (M - 1)
NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")


def make_scene(torch, P, dev):
    gen = torch.Generator(device=dev).manual_seed(5)
    shapes = {"xyz": (P, 3), "f_dc": (P, 1, 3), "f_rest": (P, M - 1, 3), "opacity": (P, 1),
              "scaling": (P, 3), "rotation": (P, 4)}
    return {k: torch.randn(s, device=dev, generator=gen) for k, s in shapes.items()}


def header(P):
    names = (["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"]
             + [f"f_rest_{i}" for i in range(3 * (M - 1))]
             + ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"])
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {P}"]
    lines += [f"property float {n}" for n in names] + ["end_header"]
    return names, ("\n".join(lines) + "\n").encode("ascii")


def restated_save(np, path, sc):
    xyz = sc["xyz"].detach().cpu().numpy()
    normals = np.zeros_like(xyz)
    f_dc = sc["f_dc"].detach().transpose(1, 2).flatten(start_dim=1).contiguous().cpu().numpy()
    f_rest = sc["f_rest"].detach().transpose(1, 2).flatten(start_dim=1).contiguous().cpu().numpy()
    opacities = sc["opacity"].detach().cpu().numpy()
    scale = sc["scaling"].detach().cpu().numpy()
    rotation = sc["rotation"].detach().cpu().numpy()
    names, head = header(xyz.shape[0])
    elements = np.empty(xyz.shape[0], dtype=[(n, "f4") for n in names])
    attributes = np.concatenate((xyz, normals, f_dc, f_rest, opacities, scale, rotation), axis=1)
    elements.view(np.float32).reshape(attributes.shape)[:] = attributes
    with open(path, "wb") as f:
        f.write(head)
        elements.tofile(f)


class PeakRss:
    """The largest growth of the resident set while the block runs (2 ms samples)."""
    PAGE = os.sysconf("SC_PAGE_SIZE")

    @classmethod
    def rss(cls):
        with open("/proc/self/statm") as f:
            return int(f.read().split()[1]) * cls.PAGE

    def __enter__(self):
        self.base = self.peak = self.rss()
        self.stop = threading.Event()
        self.thread = threading.Thread(target=self._run, daemon=True)
        self.thread.start()
        return self

    def _run(self):
        while not self.stop.wait(0.002):
            self.peak = max(self.peak, self.rss())

    def __exit__(self, *exc):
        self.stop.set()
        self.thread.join()
        self.peak = max(self.peak, self.rss())
        self.mb = (self.peak - self.base) / 2 ** 20


def pick_dir(need_bytes):
    shm = "/dev/shm"
    if os.path.isdir(shm) and os.access(shm, os.W_OK) and shutil.disk_usage(shm).free > need_bytes:
        return shm
    return os.getcwd()


def kernel_stats(d, P_list, chunk_rows):
    paths = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not paths:
        raise SystemExit(f"no *kernel_stats.csv under {d}")
    calls, total_ns = 0, 0.0
    for path in paths:
        for r in csv.DictReader(open(path)):
            if "k_ply_pack" in r["Name"]:
                calls += int(r["Calls"])
                total_ns += float(r["TotalDurationNs"])
    if not calls:
        raise SystemExit("the trace has no k_ply_pack")
    P = P_list[0]
    chunks = -(-P // chunk_rows)
    saves = calls / chunks
    floor_bytes = 2 * 4 * R * P
    per_save_ms = total_ns / saves / 1e6
    print(json.dumps(dict(kernel="k_ply_pack", P=P, chunk_rows=chunk_rows, launches=calls,
                          saves=round(saves, 3), launch_us=round(total_ns / calls / 1e3, 3),
                          per_save_ms=round(per_save_ms, 4), floor_bytes=floor_bytes,
                          gb_per_s=round(floor_bytes / per_save_ms / 1e6, 1),
                          share_of_6300_gb_per_s=round(floor_bytes / per_save_ms / 1e6 / 6300, 3))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, nargs="+", default=[1_000_000, 6_000_000])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--paths", nargs="+", default=["hip", "restated"], choices=["hip", "restated"])
    ap.add_argument("--dir", default=None)
    ap.add_argument("--kernel-stats", default=None, metavar="DIR")
    args = ap.parse_args()
    if args.kernel_stats:
        return kernel_stats(args.kernel_stats, args.P, 65536)

    import numpy as np
    import torch

    from gaussiansplattingviewer_amd import save_ply
    if not torch.cuda.is_available():
        raise SystemExit("bench_ply_save.py needs a HIP device")
    dev = torch.device("cuda", 0)
    for P in args.P:
        file_bytes = len(header(P)[1]) + 4 * R * P
        d = args.dir or pick_dir(2 * file_bytes + (1 << 30))
        files = {p: os.path.join(d, f"bench_ply_save_{os.getpid()}_{p}.ply") for p in args.paths}
        sc = make_scene(torch, P, dev)
        torch.cuda.synchronize()
        run = {"hip": lambda path: save_ply(path, sc),
               "restated": lambda path: restated_save(np, path, sc)}
        times = {p: [] for p in args.paths}
        peaks = {p: [] for p in args.paths}
        same = None
        try:
            for it in range(args.warmup + args.steps):
                for p in args.paths:
                    torch.cuda.synchronize()
                    with PeakRss() as peak:
                        t0 = time.perf_counter()
                        run[p](files[p])
                        torch.cuda.synchronize()
                        dt = time.perf_counter() - t0
                    assert os.path.getsize(files[p]) == file_bytes
                    if it >= args.warmup:
                        times[p].append(dt)
                        peaks[p].append(peak.mb)
                if it == 0 and len(args.paths) == 2:
                    with open(files["hip"], "rb") as a, open(files["restated"], "rb") as b:
                        same = all(x == y for x, y in iter(
                            lambda: (a.read(1 << 24), b.read(1 << 24)), (b"", b"")))
        finally:
            for f in files.values():
                if os.path.exists(f):
                    os.remove(f)
        for p in args.paths:
            t = times[p]
            line = dict(path=p, P=P, sh_degree=3, dir=d, file_mb=round(file_bytes / 2 ** 20, 1),
                        steps=len(t),
                        call_s=dict(median=round(statistics.median(t), 4),
                                    min_max=[round(min(t), 4), round(max(t), 4)]),
                        file_gb_per_s=round(file_bytes / statistics.median(t) / 1e9, 3),
                        peak_host_mb=round(max(peaks[p]), 1))
            if p == "restated" and "hip" in times:
                line["ratio_to_hip"] = round(statistics.median(t) / statistics.median(times["hip"]), 2)
                line["files_identical"] = same
            print(json.dumps(line), flush=True)
        del sc
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
