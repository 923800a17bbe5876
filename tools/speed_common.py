"""What the frame utilities' speed tools (csc_speed, scale_speed, ssim_speed,
lookahead_speed, tf_speed) share: device-event timing, its figures, the result
line, and the child process with one alarm per step."""
import json
import os
import signal
import subprocess
import sys


def timed(torch, fn, launches, reps, warmup=2):
    """Milliseconds per call, ascending: device events around `launches` back-to-back calls, `reps` times."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / launches)
    ms.sort()
    return ms


def rates(nbytes, ms, ms_range=False):
    gb = [nbytes / (t * 1e-3) / 1e9 for t in ms]  # ms ascending -> rates descending
    res = {"ms_median": ms[len(ms) // 2]}
    if ms_range:
        res.update({"ms_min": ms[0], "ms_max": ms[-1]})
    res.update({"gbps_median": gb[len(gb) // 2], "gbps_min": gb[-1], "gbps_max": gb[0]})
    return res


def timed_step(torch, fn, nbytes, a, ms_range=False):
    """rates() of one step of a worker under the step's own limit: the alarm ends the process."""
    signal.alarm(a.step_seconds)
    res = rates(nbytes, timed(torch, fn, a.launches, a.reps), ms_range)
    signal.alarm(0)
    return res


def write_result(res, out):
    """The result as one JSON line, printed last and written to `out` if given."""
    line = json.dumps(res)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")
    print(line)


def run_worker(tool, script, step_seconds, limit):
    """Run `script --worker` with this process's arguments in a child (one session, one set of buffers) and
    leave with its exit status; the parent gives up after `limit` seconds."""
    try:
        rc = subprocess.run([sys.executable, os.path.abspath(script), "--worker"] + sys.argv[1:], timeout=limit).returncode
    except subprocess.TimeoutExpired:
        raise SystemExit("%s: the measurement did not finish in %d s" % (tool, limit))
    if rc == -signal.SIGALRM:
        raise SystemExit("%s: a step ran past its %d s limit" % (tool, step_seconds))
    raise SystemExit(rc)
