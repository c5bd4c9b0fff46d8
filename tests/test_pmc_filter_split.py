"""CPU test of pmc_summary's split of the dense merge's launches once the store merges by its 32-bit shadow: the first
launch after the synthesis (k_merge_dense<8>), the build launch (k_merge_build) and the steady ones (k_merge_filtered),
by kernel name in dispatch order.  Synthetic rocprofv3 CSV, no GPU."""
import csv
import importlib.util
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_filter_split_names_first_build_and_steady(tmp_path):
    spec = importlib.util.spec_from_file_location("pmc_summary", ROOT / "janus-crdt_amd" / "tools" / "pmc_summary.py")
    ps = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ps)
    seq = [("k_synth_pnc", 5), ("void k_merge_dense<8>(x)", 900), ("void jg::filt::k_merge_build<256>(x)", 700),
           ("void jg::filt::k_merge_filtered<2, 1, 512>(x)", 10), ("void k_merge_dense<4>(x)", 77),
           ("void jg::filt::k_merge_filtered<2, 1, 512>(x)", 12)]
    path = tmp_path / "run_counter_collection.csv"
    with open(path, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=["Dispatch_Id", "Kernel_Name", "Counter_Name", "Counter_Value"])
        w.writeheader()
        for i, (k, v) in reversed(list(enumerate(seq))):  # rows out of dispatch order
            w.writerow({"Dispatch_Id": i + 1, "Kernel_Name": k, "Counter_Name": "FETCH_SIZE", "Counter_Value": v})
            w.writerow({"Dispatch_Id": i + 1, "Kernel_Name": k, "Counter_Name": "OTHER", "Counter_Value": 1})
    out = ps.filter_split(path, "FETCH_SIZE")
    assert out == {"first": [900 * 1024], "build": [700 * 1024], "steady": [10 * 1024, 12 * 1024]}
    # a parent's run (k_merge_dense only) has no steady filtered launch: the summary then keeps dense_split's figures
    assert ps.dense_split(path, "FETCH_SIZE") == {"first": [900 * 1024], "steady": []}
