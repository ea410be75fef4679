#!/usr/bin/env python3
"""What a checkpoint and a session file cost on C3's frame (stand-in, 1920x1080, 3 bounces).

  session_cost.py                     the workload.  One accumulator with 8 samples, no frozen pixel and no estimator
                                      (so both files hold the same records; compared byte for byte), then after a
                                      warm-up round REPS rounds of {pt_accum_save, pt_session_save} alternated and REPS
                                      rounds of {pt_accum_load, pt_session_load} alternated, all in one directory; then
                                      an accumulator after the adaptive loop (4-spp passes to 32, tolerance 0.2) with
                                      its estimator: REPS rounds of {pt_session_save, pt_session_load} with all four
                                      sections.  PT_TIMING=1 makes the library print the host wall time of each stage
                                      (state <-> host buffer, file write / read; every stage ends in a blocking call);
                                      this script collects those lines and prints one JSON line.
  session_cost.py --report RUN.json [TRACE.csv]
                                      medians and ranges per stage (the warm-up round dropped), the comparison the
                                      design rests on -- pt_session_save's state-to-host stage against pt_accum_save's
                                      in the same run, with the spread of the latter's repeats as the margin -- and,
                                      with a kernel trace of a second run, the pack / unpack kernels against their
                                      traffic floors: (bytes read once + bytes written once) / 8 TB/s.
Bytes per work slot: pack and unpack move the slot -> pixel map 4, the rng words 24 and the mean 24 one way and the
48-B record the other (100 B); with all four sections also frozen_at 4, the estimator's planes 40 and W_q / b_q 8,
and their records 4 + 40 + 8 (204 B)."""
import json
import os
import re
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

W, H, BOUNCES = 1920, 1080, 3
REPS = int(os.environ.get("REPS", "7"))
PEAK = 8e12
BYTES = {"plain": 100, "full": 204}
LOOP = dict(pass_spp=4, max_samples=32, tol=0.2, quantile=1.0, min_batches=2)
LINE = re.compile(r"^(pt_\w+): (.+?)\s+([0-9.]+) ms$")


class Stages:
    """The library's PT_TIMING lines of one call, read from the process's stderr (fd 2)."""

    def __init__(self):
        self.tmp = tempfile.TemporaryFile(mode="w+b")

    def call(self, fn):
        sys.stderr.flush()
        keep = os.dup(2)
        self.tmp.seek(0)
        self.tmp.truncate()
        os.dup2(self.tmp.fileno(), 2)
        try:
            t = time.perf_counter()
            r = fn()
            wall = (time.perf_counter() - t) * 1e3
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        self.tmp.seek(0)
        out = {"wall": wall}
        for ln in self.tmp.read().decode(errors="replace").splitlines():
            m = LINE.match(ln.strip())
            if m:
                out[m.group(2).strip()] = float(m.group(3))
            else:
                sys.stderr.write(ln + "\n")
        return r, out


def same_records(fa, fs):
    a, s = open(fa, "rb"), open(fs, "rb")
    a.seek(128)
    s.seek(192)
    while True:
        x, y = a.read(1 << 24), s.read(1 << 24)
        if x != y:
            return False
        if not x:
            return True


def run():
    os.environ["PT_TIMING"] = "1"
    import cudapathtracer_amd as pt
    from cudapathtracer_amd import scenes
    d = os.path.join(tempfile.gettempdir(), "pt_bench_scene")
    p = os.path.join(d, "models", "sponza_standin.obj")
    if not os.path.exists(p):
        scenes.write_sponza_standin(d)
    s = pt.Scene()
    s.load_obj(p, mtl_basepath=os.path.dirname(p) + "/")
    s.build_bvh()
    cam = pt.make_camera(width=W, height=H, **scenes.SPONZA_STANDIN_CAMERA)
    work = tempfile.mkdtemp(prefix="pt_session_cost_")
    fa, fs, ff = (os.path.join(work, n) for n in ("a.ptacc", "s.ptses", "full.ptses"))
    st = Stages()
    calls = {k: [] for k in ("accum_save", "session_save", "accum_load", "session_load", "session_save_full", "session_load_full")}
    info = {}
    try:
        with pt.Renderer(s, 0) as r:
            r.render(cam, W, H, 2, bounces=BOUNCES)   # warm-up: jump tables, buffers
            with r.accumulator(cam, W, H, bounces=BOUNCES) as acc:
                acc.add(8)
                for rep in range(REPS + 1):   # (rep 0: warm-up)
                    calls["accum_save"].append(st.call(lambda: acc.save(fa))[1])
                    calls["session_save"].append(st.call(lambda: acc.save_session(fs))[1])
                if not same_records(fa, fs):
                    sys.exit("session_cost: section A differs from the checkpoint's records")
                want = acc.mean64().tobytes()
            for rep in range(REPS + 1):
                a, t = st.call(lambda: r.load_accumulator(fa))
                calls["accum_load"].append(t)
                ok = rep or a.mean64().tobytes() == want
                a.close()
                (b, _), t = st.call(lambda: r.load_session(fs))
                calls["session_load"].append(t)
                ok = ok and (rep or b.mean64().tobytes() == want)
                b.close()
                if not ok:
                    sys.exit("session_cost: a loaded accumulator differs from the saved one")
            info["file_bytes"] = {"checkpoint": os.path.getsize(fa), "session": os.path.getsize(fs)}
            with r.accumulator(cam, W, H, bounces=BOUNCES) as acc:
                res = acc.add_adaptive(**LOOP)
                est = acc._noise
                for rep in range(REPS + 1):
                    calls["session_save_full"].append(st.call(lambda: acc.save_session(ff, est))[1])
                want = (acc.mean64().tobytes(), acc.counts().tobytes(), est.read()[1].tobytes())
            info["adaptive"] = {k: res[k] for k in ("passes", "active", "samples_total", "stopped_converged")}
            info["file_bytes"]["session_full"] = os.path.getsize(ff)
            info["full_flags"] = pt.session_file_info(ff)["flags"]
            info["frozen_pixels"] = pt.session_file_info(ff)["frozen_pixels"]
            for rep in range(REPS + 1):
                (b, e), t = st.call(lambda: r.load_session(ff))
                calls["session_load_full"].append(t)
                if not rep and (b.mean64().tobytes(), b.counts().tobytes(), e.read()[1].tobytes()) != want:
                    sys.exit("session_cost: the loaded adaptive state differs from the saved one")
                b.close()
    finally:
        shutil.rmtree(work, ignore_errors=True)
    print(json.dumps({"config": [W, H, BOUNCES], "reps": REPS, "info": info,
                      "ms_first_is_warmup": calls}))
    if info["full_flags"] != 7:
        sys.exit("session_cost: the adaptive state did not produce all four sections")


def report(run_json, trace=None):
    info = json.loads(open(run_json).read().strip().splitlines()[-1])
    out = {"image": info["config"][:2], "reps": info["reps"], "info": info["info"], "stages_ms_median_min_max": {}}
    tab = out["stages_ms_median_min_max"]
    for call, reps in info["ms_first_is_warmup"].items():
        reps = reps[1:]
        tab[call] = {}
        for stage in reps[0]:
            v = [x[stage] for x in reps]
            tab[call][stage] = "%.3f %.3f %.3f" % (statistics.median(v), min(v), max(v))
    num = lambda call, stage: [float(x) for x in tab[call][stage].split()]   # noqa: E731
    a, s_ = num("accum_save", "state to host"), num("session_save", "state to host")
    out["state_to_host"] = {"pt_accum_save_median_ms": a[0], "pt_accum_save_spread_ms": round(a[2] - a[1], 3),
                            "pt_session_save_median_ms": s_[0],
                            "session_not_slower_within_spread": s_[0] <= a[0] + (a[2] - a[1]),
                            "ratio": round(a[0] / s_[0], 2)}
    a, s_ = num("accum_load", "host to state"), num("session_load", "host to state")
    out["host_to_state"] = {"pt_accum_load_median_ms": a[0], "pt_session_load_median_ms": s_[0], "ratio": round(a[0] / s_[0], 2)}
    if trace:
        import csv
        rows = sorted(csv.DictReader(open(trace)), key=lambda r: int(r["Start_Timestamp"]))
        us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3   # noqa: E731
        slots = ((W + 7) // 8) * ((H + 7) // 8) * 64
        n = info["reps"] + 1
        out["kernels"] = {"slots": slots}
        for kern in ("session_pack", "session_unpack"):
            t = [us(r) for r in rows if kern + "_planes" in r["Kernel_Name"]]
            assert len(t) == 2 * n, (kern, len(t))
            for kind, part in (("plain", t[:n][1:]), ("full", t[n:][1:])):   # (the first of each: warm-up)
                floor = slots * BYTES[kind] / PEAK * 1e6
                m = statistics.median(part)
                out["kernels"]["%s_%s" % (kern, kind)] = {"us": [round(x, 1) for x in part], "median_us": round(m, 1),
                                                           "bytes_per_slot": BYTES[kind], "traffic_floor_us": round(floor, 2),
                                                           "over_floor": round(m / floor, 2)}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "--report":
        report(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    else:
        run()
