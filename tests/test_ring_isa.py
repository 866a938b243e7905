"""What the gfx950 ISA of the headline kernel, k_fused_ring<2, Log1p(1.5), grad, codebook stream>, must show (no GPU
needed): the accumulator read-ahead of the consumer loop and the batched combine of the in-launch fold."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "_Z12k_fused_ringILi2E8FnSingleILi9ELi2EELb1ELi1ELb1EE"   # <2, FnSingle<LOG1P, 2>, true, 1, true>
GR_OFF = (7816 + 32) * 8 + 256                                     # ring_gr_off(2): the accumulators' LDS offset


@pytest.fixture(scope="module")
def body(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("isa") / "k.s"
    pr = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                         "-ffp-contract=fast", "-S", "--cuda-device-only",
                         os.path.join(ROOT, "pymde_amd", "csrc", "mde_ring_k_log1p.hip"), "-o", str(out)],
                        stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert pr.returncode == 0, pr.stdout.decode(errors="replace")[-2000:]
    lines = out.read_text().split("\n")
    s = next(i for i, l in enumerate(lines) if l.startswith(KERNEL) and l.split()[0].endswith(":"))
    e = next(i for i in range(s, len(lines)) if "s_endpgm" in lines[i])
    return [l.split(";")[0].strip() for l in lines[s + 1:e]]


def test_consumer_reads_both_accumulators_of_a_pair_before_writing_either(body):
    """Per basic block, the accumulator accesses go R R W W R R W W ...: no accumulator read sits between the two
    writes of a pair (the read of the second entry behind the first one's write cost an exposed LDS round trip
    per pair, which drained the next pair's operand reads with it)."""
    seq, pairs = [], 0
    for t in body + [".LBB_end:"]:
        if re.match(r"^\.LBB\d+_\d+:|^\.LBB_end:", t) or t.startswith(("s_cbranch", "s_branch")):
            s = "".join(seq)
            assert not re.search("WR+W", s), "an accumulator read between two writes in a basic block: " + s
            pairs += s.count("WWRR")
            seq = []
            continue
        if ("offset:%d" % GR_OFF) in t:
            if t.startswith("ds_read_b64"):
                seq.append("R")
            elif t.startswith("ds_write_b64"):
                seq.append("W")
    # 3 stream blocks x 3 loss classes x 2 pairs, less the regions that end at a block's branch
    assert pairs >= 8, pairs


def test_fold_combine_issues_its_device_scope_loads_in_batches(body):
    """Every loop that reads the other column group's partial rows (device-scope loads, sc1) and writes gradient rows
    issues at least eight of those loads per trip -- not one load and a vmcnt(0) per trip.  (The flag poll and the
    last workgroup's sum of the loss partials store nothing.)"""
    labels = {t[:-1]: i for i, t in enumerate(body) if re.match(r"^\.LBB\d+_\d+:$", t)}
    loops = 0
    for i, t in enumerate(body):
        m = re.match(r"^s_cbranch_\w+\s+(\.LBB\d+_\d+)$", t)
        if not m or labels.get(m.group(1), i + 1) > i:
            continue
        trip = body[labels[m.group(1)]:i + 1]
        loads = [x for x in trip if x.startswith("global_load") and x.endswith("sc1")]
        if not loads or not any(x.startswith("global_store") for x in trip):
            continue
        loops += 1
        assert len(loads) >= 8, "a combine loop with %d device-scope loads per trip:\n%s" % (len(loads), "\n".join(trip))
    assert loops >= 2, loops   # (the contiguous and the dealt-row paths)
