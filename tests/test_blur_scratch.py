"""The view of the depth blur's two weight scratch buffers (cs_kernels.h BlurScratch): every member lies where launch_blur and
launch_gray_edges used to find it by pointer arithmetic at the call site, and whatever form a call is planned in -- fused, listed,
lazy -- keeps every part inside the al256(n * h * w * 4) bytes each buffer holds.  No GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BLUR_SCRATCH_SRC = r'''
#include <stdio.h>
#include <stdlib.h>
#include "cs_kernels.h"
using cs::al256;
struct Part { const char* name; int buf; size_t off, bytes; bool used; };   // buf 0: wl, 1: wr
int main() {
    const int ws[] = {1, 2, 3, 4, 8, 63, 64, 65, 130, 1284, 3840}, hs[] = {1, 5, 31, 32, 33, 100, 2160}, ns[] = {1, 3, 64};
    int bad = 0, cases = 0, fused = 0, listed = 0, lazy = 0;
    for (int w : ws) for (int h : hs) for (int n : ns) for (int planes = 1; planes <= 2; planes++) {
        const size_t buf = al256((size_t)n * h * w * 4);
        char* wl = (char*)aligned_alloc(256, buf);
        char* wr = (char*)aligned_alloc(256, buf);
        if (!wl || !wr) { printf("no memory\n"); return 2; }
        const cs::BlurScratch S = cs::blur_scratch((float*)wl, (float*)wr, n, h, w, planes);
        const cs::BlurScratch Z = cs::blur_scratch(nullptr, nullptr, n, h, w, planes);
        // the geometry and the offsets as blur_plan and the call sites spelled them before there was a view
        const int MW = (w + 63) / 64, gy = (h + 32 - 1) / 32, gx = (w + 64 - 1) / 64, HB = (h + 4 - 1) / 4;
        const size_t plane_bytes = ((size_t)n * h * MW * 8 + 255) & ~(size_t)255, mask_bytes = plane_bytes * planes;
        const size_t total = (size_t)n * gy * gx;
        const size_t list_bytes = 256 + ((total * 4 + 15) & ~(size_t)15) + total * 64, blk_bytes = (size_t)n * HB * MW * 16;
        bad += S.MW != MW || S.gy != gy || S.gx != gx || S.HB != HB || S.tiles != total;
        bad += (char*)S.wl != wl || (char*)S.wr != wr || (char*)S.bits_l != wl || (char*)S.bits_r != wr;
        bad += S.plane_words != plane_bytes / 8;
        bad += (char*)S.work_count != wl + mask_bytes;
        bad += S.worklist != S.work_count + 64;
        bad += (char*)S.tile_stats != (char*)S.worklist + ((total * 4 + 15) & ~(size_t)15);
        bad += (char*)S.block_summaries != wr + mask_bytes;
        bad += S.listed_bytes != mask_bytes + list_bytes || S.lazy_bytes != mask_bytes + blk_bytes || S.buf_bytes != buf;
        // the predicates as blur_plan spelled them; the fused one is new: before, the fused form was taken whatever its bit rows needed
        const size_t room = (size_t)n * h * w * 4;
        bad += S.fits_listed != (S.fits_fused && gx < 1024 && gy < 1024 && n < 4096 && mask_bytes + list_bytes <= room);
        bad += S.fits_lazy != (S.fits_listed && mask_bytes + blk_bytes <= room);
        // one plane: the bit rows of a one-column frame of more than 32 rows outgrow the buffer, and no others
        if (planes == 1) bad += S.fits_fused != !(w == 1 && (size_t)n * h > 32);
        // base pointers null: the same numbers, no pointer
        bad += Z.bits_l || Z.bits_r || Z.work_count || Z.worklist || Z.tile_stats || Z.block_summaries || Z.wl || Z.wr;
        bad += Z.plane_words != S.plane_words || Z.listed_bytes != S.listed_bytes || Z.lazy_bytes != S.lazy_bytes || Z.bits_bytes != S.bits_bytes ||
               Z.fits_fused != S.fits_fused || Z.fits_listed != S.fits_listed || Z.fits_lazy != S.fits_lazy;
        // what the kernels write through each member, by the form that uses it (two planes: the lazy form is their one consumer)
        const bool use_fused = planes == 1 ? S.fits_fused : S.fits_lazy, use_listed = use_fused && S.fits_listed;
        const size_t rows_bytes = (size_t)n * h * MW * 8;
        auto off = [&](const void* p, const char* base) { return (size_t)((const char*)p - base); };
        const Part parts[] = {
            {"bits_l plane 0", 0, 0, rows_bytes, use_fused},
            {"bits_l plane 1", 0, S.plane_words * 8, planes == 2 ? rows_bytes : 0, use_fused && planes == 2},
            {"work_count", 0, off(S.work_count, wl), 256, use_listed},
            {"worklist", 0, off(S.worklist, wl), total * 4, use_listed},
            {"tile_stats", 0, off(S.tile_stats, wl), total * 64, use_listed},
            {"bits_r plane 0", 1, 0, rows_bytes, use_fused},
            {"bits_r plane 1", 1, S.plane_words * 8, planes == 2 ? rows_bytes : 0, use_fused && planes == 2},
            {"block_summaries", 1, off(S.block_summaries, wr), blk_bytes, S.fits_lazy}};
        const int np = sizeof(parts) / sizeof(parts[0]);
        bad += S.bits_bytes != (planes - 1) * plane_bytes + rows_bytes;
        bad += off(S.tile_stats, wl) % 16 != 0 || off(S.block_summaries, wr) % 16 != 0 || off(S.work_count, wl) % 256 != 0;
        for (int i = 0; i < np; i++) {
            for (int j = 0; j < i; j++)   // disjoint, whether the form is taken or not
                if (parts[i].buf == parts[j].buf && parts[i].off < parts[j].off + parts[j].bytes && parts[j].off < parts[i].off + parts[i].bytes) {
                    printf("%s overlaps %s\n", parts[i].name, parts[j].name); bad++;
                }
            if (!parts[i].used) continue;
            if (parts[i].off + parts[i].bytes > buf) { printf("%s outside its buffer\n", parts[i].name); bad++; continue; }
            char* base = parts[i].buf ? wr : wl;   // (under the sanitizer: inside the allocation)
            base[parts[i].off] = (char)i; base[parts[i].off + parts[i].bytes - 1] = (char)i;
        }
        free(wl); free(wr);
        if (bad) { printf("n = %d, h = %d, w = %d, planes = %d: %d failures\n", n, h, w, planes, bad); return 1; }
        cases++; fused += planes == 1 && S.fits_fused; listed += S.fits_listed; lazy += S.fits_lazy;
    }
    printf("ok %d %d %d %d\n", cases, fused, listed, lazy);
    return 0;
}
'''


def test_blur_scratch_members_lie_where_the_kernels_find_them(tmp_path):
    """cs_kernels.h's view of wl / wr in a stand-alone host program under AddressSanitizer and UBSan, over 11 widths x 7 heights x
    3 batch sizes x 1 or 2 bit-row planes: every member at the offset the call sites used to compute by hand, listed_bytes and
    lazy_bytes the sums blur_plan compared, the members disjoint, and every part of a form the view lets a plan take inside
    the buffer -- the program writes each part's first and last byte into allocations of exactly that size.  The fused form is
    refused exactly for one-column frames of more than 32 rows, the only shapes whose (one-plane) bit rows outgrow the buffer."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = tmp_path / "blur_scratch.hip"
    src.write_text(BLUR_SCRATCH_SRC)
    exe = tmp_path / "blur_scratch"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "comfystereo_amd", "csrc"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    word, cases, fused, listed, lazy = out.stdout.split()
    # 15 of the 21 one-column shapes have more than 32 rows in all; some shapes take each of the further forms
    assert word == "ok" and int(cases) == 11 * 7 * 3 * 2 and int(fused) == int(cases) // 2 - 15 and 0 < int(lazy) < int(listed)
