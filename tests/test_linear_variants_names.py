"""The profile scripts' kernel-name handling after igemm_dma_kernel gained two trailing template arguments (the linear form and the
epilogue kind, written by rocprofv3 as `..., true, (maa::Epi)1>`): old and new spellings land on the same bench / profile row, and
the summaries cut a name at its parameter list, not at the cast inside the template arguments."""
import json
import os
import sqlite3
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OLD = "igemm_dma_kernel<64, 64, 2, 2, 2, 3>"
NEW = "igemm_dma_kernel<64, 64, 2, 2, 2, 3, true, (maa::Epi)1>"
NEW_SPLIT = "igemm_dma_kernel<128, 64, 2, 2, 3, 3, true, (maa::Epi)2>"


def test_old_and_new_kernel_names_resolve_to_the_same_traffic_rows(tmp_path):
    txt = tmp_path / "pmc.txt"
    txt.write_text(
        "== FETCH_SIZE GRBM_GUI_ACTIVE  (4 DDIM steps)\n"
        "%-60s grid 249600    launches   100  FETCH_SIZE=500000  GRBM_GUI_ACTIVE=1\n"
        "%-60s grid 249600    launches   100  FETCH_SIZE=500000  GRBM_GUI_ACTIVE=1\n"
        "%-60s grid 125440    launches    40  FETCH_SIZE=100000  GRBM_GUI_ACTIVE=1\n"
        "== WRITE_SIZE GRBM_GUI_ACTIVE  (4 DDIM steps)\n"
        "%-60s grid 249600    launches   100  WRITE_SIZE=250000  GRBM_GUI_ACTIVE=1\n"
        "%-60s grid 249600    launches   100  WRITE_SIZE=250000  GRBM_GUI_ACTIVE=1\n"
        "%-60s grid 125440    launches    40  WRITE_SIZE=80000  GRBM_GUI_ACTIVE=1\n" % (OLD, NEW, NEW_SPLIT, OLD, NEW, NEW_SPLIT))
    out = str(tmp_path / "t.json")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "pmc_traffic_json.py"), str(txt), "bf16x3", "4", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    k = json.load(open(out))["kernels"]
    assert k["igemm_dma_bf16x3<64x64>"]["launches"] == 200
    assert abs(k["igemm_dma_bf16x3<64x64>"]["hbm_bytes_per_launch"] - (2 * 1000000 + 500000) * 1024.0 / 200) < 1e-6
    assert k["igemm_dma_bf16x3<128x64>"]["launches"] == 40


def test_summaries_keep_the_template_arguments_of_the_new_names(tmp_path):
    full = "void maa::(anonymous namespace)::%s(maa::IGemm, int, int, unsigned int)" % NEW
    # the shapes script reads the `kernels` view, the counter summary `counters_collection`
    db = str(tmp_path / "r.db")
    con = sqlite3.connect(db)
    con.execute("create table kernels (name text, grid_x int, grid_y int, duration real)")
    con.execute("insert into kernels values (?, 256000, 1, 50000.0)", (full,))
    con.execute("create table counters_collection (kernel_name text, counter_name text, grid_size_x int, value real)")
    con.execute("insert into counters_collection values (?, 'SQ_WAVES', 256000, 4000.0)", (full,))
    con.commit()
    con.close()
    for script in ("rocprof_shapes.py", "pmc_summary.py"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script), db], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert NEW + " " in r.stdout, (script, r.stdout)
        assert "maa::IGemm" not in r.stdout, (script, r.stdout)
