"""The host half of the motion-compensated depth filter (csrc/cs_motiondepth.h) in a stand-alone program under AddressSanitizer and
UBSan, on the CPU: the parameters' refusals, the workspace's blocks and the packed key of the search order."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <tuple>
#include "cs_motiondepth.h"
using namespace cs;

int main() {
    int bad = 0;
    // the parameters' ranges
    bad += motion_args_error(0, 0, 0) != nullptr || motion_args_error(32, 4096, 255) != nullptr;
    bad += !motion_args_error(-1, 0, 0) || !motion_args_error(33, 0, 0) || !motion_args_error(0, -1, 0) || !motion_args_error(0, 4097, 0);
    bad += !motion_args_error(0, 0, -1) || !motion_args_error(0, 0, 256) || !strstr(motion_args_error(40, -1, 999), "search_range");
    if (bad) { printf("parameter checks: %d failures\n", bad); return 1; }
    // the key orders like the tuple, over every vector and costs that tie and differ, the largest cost included
    const uint32_t costs[] = {0u, 1u, 2u, 65280u, 255u * 256u + 4096u * 64u};
    uint64_t prev_key = 0;
    std::tuple<uint32_t, int, int, int, int> prev_tuple;
    bool first = true;
    for (uint32_t cost : costs)
        for (int mag = 0; mag <= 64; mag++)
            for (int ady = 0; ady <= 32 && ady <= mag; ady++)
                for (int sy = -1; sy <= 1; sy += 2)
                    for (int sx = -1; sx <= 1; sx += 2) {   // tuples in ascending order: (cost, mag, |dy|, dy, dx)
                        const int adx = mag - ady;
                        if (adx > 32 || (ady == 0 && sy > 0) || (adx == 0 && sx > 0)) continue;
                        const int dy = sy * ady, dx = sx * adx;
                        const uint64_t key = motion_key(cost, dx, dy);
                        const auto tuple = std::make_tuple(cost, mag, ady, dy, dx);
                        if (!first && !(prev_tuple < tuple && prev_key < key)) { printf("order broken at cost %u (%d, %d)\n", cost, dx, dy); bad++; }
                        int rx, ry; int32_t sad;
                        motion_unkey(key, 4096, &rx, &ry, &sad);
                        if (rx != dx || ry != dy || sad != (int32_t)cost - 4096 * mag) { printf("round trip broken at (%d, %d)\n", dx, dy); bad++; }
                        if (key >> 46) { printf("key wider than 46 bits\n"); bad++; }
                        prev_key = key; prev_tuple = tuple; first = false;
                    }
    if (bad) return 1;
    // the workspace: blocks on 256-byte boundaries, disjoint, inside the size the library asks for, large enough for their users
    const int shapes[][3] = {{1, 1, 1}, {1, 16, 16}, {3, 17, 33}, {2, 50, 70}, {64, 130, 258}, {2, 129, 128}};
    for (const auto& s : shapes) {
        const int n = s[0], h = s[1], w = s[2];
        const size_t hw = (size_t)h * w;
        const MotionViews S = motion_views(nullptr, n, h, w);
        uint8_t* base = (uint8_t*)aligned_alloc(256, S.bytes);
        const MotionViews V = motion_views(base, n, h, w);
        bad += V.bytes != S.bytes || S.partial || S.luma || S.yprev || V.pitch % 4 || V.pitch < (size_t)w || V.pitch > (size_t)w + 3;
        const size_t off[3] = {(size_t)((uint8_t*)V.partial - base), (size_t)(V.luma - base), (size_t)((uint8_t*)V.yprev - base)};
        const size_t len[3] = {(size_t)n * temporal_partials(hw) * 4, ((size_t)n + 1) * h * V.pitch, hw * 4};
        for (int i = 0; i < 3; i++) {
            bad += off[i] % 256 != 0 || off[i] + len[i] > V.bytes;
            for (int j = 0; j < i; j++) bad += off[i] < off[j] + len[j] && off[j] < off[i] + len[i];
            memset(base + off[i], i, len[i]);   // (under the sanitizer: inside the allocation)
        }
        free(base);
        if (bad) { printf("workspace of %d x %d x %d: %d failures\n", n, h, w, bad); return 1; }
    }
    bad += motion_blocks(1) != 1 || motion_blocks(16) != 1 || motion_blocks(17) != 2 || motion_blocks(258) != 17;
    bad += MD_PITCH_DW != 33 || MD_ROWS != 80;
    if (bad) return 1;
    printf("ok\n");
    return 0;
}
'''


def test_parameter_checks_workspace_blocks_and_key_packing_under_the_sanitizers(tmp_path):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = tmp_path / "motion_host.hip"
    src.write_text(SRC)
    exe = tmp_path / "motion_host"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "comfystereo_amd", "csrc"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
