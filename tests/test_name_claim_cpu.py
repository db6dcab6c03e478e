"""The claim protocol of the device-side barcode dictionary (hast_amd/csrc/name_claim.h, the code k_fq_name_claim steps) under a
scheduler that enumerates every interleaving of the lanes' memory operations (tests/native/test_name_claim.cpp): one answer per text,
dense ids, consistent entries, no slot left half written -- in every complete schedule of every configuration; and the checker must
catch the order shipped up to round 10 (counter looked at after the state, no second look), which it carries as a variant."""
import os
import re
import subprocess

from tests.conftest import ROOT


def test_name_claim_protocol_every_schedule(tmp_path):
    exe = tmp_path / "test_name_claim"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", "test_name_claim.cpp")], check=True)
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    out = r.stdout.decode()
    print(out)
    assert r.returncode == 0, (out[-1500:], r.stderr.decode()[-2000:])
    rows = {ln.split()[0]: ln for ln in out.splitlines() if "shipped:" in ln}
    # the configurations the protocol has to be shown in
    for name in ("TT_limit1", "TTU_limit1_same_home", "TTU_limit1_other_home", "TTU_limit2", "TUV_limit2", "TTUU_limit1", "TTUU_limit2",
                 "wrap_TTU_2slots_limit1", "wrap_TUV_4slots_limit2", "two_kernels_limit1", "two_kernels_limit2"):
        m = re.search(r"shipped: (\d+) schedules, (\d+) bad, (\d+) states, (\d+) cuts \| r6: (\d+) schedules, (\d+) bad", rows[name])
        assert m, rows[name]
        assert int(m.group(1)) > 100 and int(m.group(2)) == 0 and int(m.group(4)) > 0, rows[name]
    # the smallest one: two lanes, one text, one id -- the old order leaves one lane with id 0 and the other with "unknown"
    m = re.search(r"r6: (\d+) schedules, (\d+) bad: two answers for one text", rows["TT_limit1"])
    assert m and 0 < int(m.group(2)) < int(m.group(1)), rows["TT_limit1"]
    last = out.strip().splitlines()[-1]
    m = re.match(r"ok shipped (\d+) schedules 0 bad; r6 (\d+) schedules (\d+) bad in (\d+) of (\d+) configurations", last)
    assert m and int(m.group(3)) > 0, last
