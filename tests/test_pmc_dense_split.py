"""CPU test of pmc_summary's split of the dense merge's launches: the first launch after the synthesis (cells raised,
lines written back) apart from the steady ones (the same batch again: reads only).  Synthetic rocprofv3 CSV, no GPU."""
import csv
import importlib.util
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_dense_split_takes_the_first_launch_apart_in_dispatch_order(tmp_path):
    spec = importlib.util.spec_from_file_location("pmc_summary", ROOT / "janus-crdt_amd" / "tools" / "pmc_summary.py")
    ps = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ps)
    seq = [("k_synth_pnc", 5), ("void k_merge_dense<8>(x)", 900), ("void k_merge_dense<8>(x)", 10), ("void k_merge_dense<4>(x)", 77),
           ("void k_merge_dense<8>(x)", 12)]
    path = tmp_path / "run_counter_collection.csv"
    with open(path, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=["Dispatch_Id", "Kernel_Name", "Counter_Name", "Counter_Value"])
        w.writeheader()
        for i, (k, v) in reversed(list(enumerate(seq))):  # rows out of dispatch order
            w.writerow({"Dispatch_Id": i + 1, "Kernel_Name": k, "Counter_Name": "WRITE_SIZE", "Counter_Value": v})
            w.writerow({"Dispatch_Id": i + 1, "Kernel_Name": k, "Counter_Name": "OTHER", "Counter_Value": 1})
    out = ps.dense_split(path, "WRITE_SIZE")
    assert out == {"first": [900 * 1024], "steady": [10 * 1024, 12 * 1024]}
