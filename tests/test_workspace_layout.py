"""The host code that carves the workspaces (cs_abi.hip, cs_kernels.h RowBlock): every size the ABI reports and every code it returns
for a refused call are the ones recorded in tests/golden/workspace_bytes.json before the carving was single-sourced, and the
flagged-row block's members lie where the kernels have always found them.  No GPU."""
import json
import os
import shutil
import subprocess
import sys

import pytest

from comfystereo_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import workspace_sizes   # noqa: E402


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "workspace_bytes.json")) as f:
        return json.load(f)


def test_every_reported_size_is_the_recorded_one(golden):
    """cs_workspace_bytes over techniques x modes x blur x depth resize x dialect flags x shapes x chunks (and the replay pool of
    pt_variant = tiny_replay_pool), and the ten per-entry-point queries over the same shapes."""
    got = workspace_sizes.sizes(_native.lib())
    assert sorted(got) == sorted(k for k in golden if k != "refused")
    for group, want in golden.items():
        if group == "refused":
            continue
        assert sorted(got[group]) == sorted(want), group
        for key, values in want.items():
            assert got[group][key] == values, (group, key)
    assert len(golden["generate"]) == 2 * (11 + 2) and all(len(v) >= 5 * 2 * 2 * 2 * 36 for v in golden["generate"].values())


def test_refused_calls_return_the_recorded_codes(golden):
    """Null pointers, non-positive sizes, over-wide rows, tensors of 2^31 elements (by shape only) and too-small workspaces, drawn
    at random for the entry points whose stats pre-pass is one helper: each is refused with the code recorded before."""
    L = _native.lib()
    seen = set()
    for entry in workspace_sizes.ENTRIES:
        want = golden["refused"][entry]
        calls = workspace_sizes.refused_calls(entry)
        assert len(calls) == len(want) and _native.CS_OK not in want
        for args, code in zip(calls, want):
            assert getattr(L, entry)(*args) == code, (entry, args)
        seen |= set(want)
    assert seen == {_native.CS_EINVAL, _native.CS_EWORKSPACE, _native.CS_ELIMIT}


ROW_BLOCK_SRC = r'''
#include <stdio.h>
#include <stdlib.h>
#include "cs_kernels.h"
using cs::al256;
struct Part { const char* name; size_t off, bytes; };
int main() {
    int bad = 0;
    const size_t all_rows[] = {1, 255, 256, 257, 260, 2160, 64 * 2160};
    for (size_t rows : all_rows) {
        const cs::RowBlock S = cs::row_block(nullptr, rows);
        uint8_t* base = (uint8_t*)aligned_alloc(256, S.bytes);
        const cs::RowBlock B = cs::row_block(base, rows);
        auto off = [&](const void* p) { return (size_t)((const uint8_t*)p - base); };
        // the offsets as the call sites spelled them before there was a view
        bad += off(B.flags) != 0;
        bad += off(B.first) != al256(rows) || off(B.retry) != al256(rows) + 8 * 4 || off(B.point2) != al256(rows) + 16 * 4;
        bad += off(B.replay_ctr) != al256(rows) + 256;
        bad += off(B.retry_flags) != al256(rows) + 512 || B.naive_flags2() != B.retry_flags;
        bad += off(B.hints) != 2 * al256(rows) + 512;
        bad += off(B.flags2) != 2 * al256(rows) + 512 + al256(rows * 8);
        bad += off(B.hints2) != 2 * al256(rows) + 512 + al256(rows * 8) + al256(rows);
        bad += B.clear_bytes != 2 * al256(rows) + 512 + al256(rows * 8) + al256(rows) + al256(rows * 8);
        bad += off(B.list) != B.clear_bytes || B.bytes != B.clear_bytes + al256(rows * 4);
        bad += S.bytes != B.bytes || S.clear_bytes != B.clear_bytes || S.flags || S.first || S.retry || S.point2 || S.list;
        // what each member's users write: pairwise disjoint (naive_flags2 is the one alias), all but the list inside the cleared part
        const Part parts[] = {{"flags", off(B.flags), rows}, {"first", off(B.first), 8}, {"retry", off(B.retry), 8}, {"point2", off(B.point2), 8},
                              {"replay_ctr", off(B.replay_ctr), 256}, {"retry_flags", off(B.retry_flags), rows}, {"hints", off(B.hints), rows * 8},
                              {"flags2", off(B.flags2), rows}, {"hints2", off(B.hints2), rows * 8}, {"list", off(B.list), rows * 4}};
        const int np = sizeof(parts) / sizeof(parts[0]);
        for (int i = 0; i < np; i++) {
            const bool is_list = i == np - 1;
            if (!is_list && parts[i].off + parts[i].bytes > B.clear_bytes) { printf("%s outside the cleared part\n", parts[i].name); bad++; }
            if (parts[i].off + parts[i].bytes > B.bytes) { printf("%s outside the block\n", parts[i].name); bad++; }
            for (int j = 0; j < i; j++)
                if (parts[i].off < parts[j].off + parts[j].bytes && parts[j].off < parts[i].off + parts[i].bytes) {
                    printf("%s overlaps %s\n", parts[i].name, parts[j].name); bad++;
                }
            for (size_t k = 0; k < parts[i].bytes; k++) base[parts[i].off + k] = (uint8_t)i;   // (under the sanitizer: inside the allocation)
        }
        free(base);
        if (bad) { printf("rows = %zu: %d failures\n", rows, bad); return 1; }
    }
    printf("ok\n");
    return 0;
}
'''


def test_row_block_members_lie_where_the_kernels_find_them(tmp_path):
    """cs_kernels.h's view of the flagged-row block in a stand-alone host program under AddressSanitizer and UBSan: every member at
    the offset the call sites used to compute by hand, the members disjoint but for the documented alias, everything but the row
    list inside clear_bytes -- for row counts at, around and far from the 256-byte padding."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = tmp_path / "row_block.hip"
    src.write_text(ROW_BLOCK_SRC)
    exe = tmp_path / "row_block"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "comfystereo_amd", "csrc"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
