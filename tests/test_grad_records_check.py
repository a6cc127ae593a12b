"""The workgroup records of the gradient un-pack (csrc/kernels.h grad_records_build) on the CPU: builds tools/grad_records_check.cpp
without sanitizers (make grad_records_check_plain) and runs it -- every element of every synthetic segment list covered by exactly
one (workgroup, thread) at its destination, as many records as the launch has workgroups.  `make grad_records_check` is the same
program under AddressSanitizer + UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hydra-gnn_amd", "csrc")


def test_record_table_covers_every_element_once():
    subprocess.run(["make", "-C", CSRC, "grad_records_check_plain"], check=True, capture_output=True, timeout=300)
    r = subprocess.run([os.path.join(CSRC, "build", "grad_records_check_plain")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "grad_records_check OK" and len(lines) == 7, r.stdout
    assert all(ln.rstrip().endswith(": ok") for ln in lines[:-1]), r.stdout
