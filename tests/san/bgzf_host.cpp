// The host build of the BGZF decoder (vireo_amd/csrc/vrx_bgzf.h, one lane) as a stand-alone program, for a
// sanitizer build: tests/test_bgzf_cpu.py compiles it with -fsanitize=address,undefined and runs it as a child.
//
//   bgzf_host CASES RESULTS
//
// CASES: records of { u32 n, n bytes }, each a file image of BGZF members.  RESULTS: per record { i32 scan status,
// u32 members }, then per member { u32 status, u32 n, n bytes of text } (n = 0 with a status).  Every image, every
// payload and every text lives in a heap block of exactly its size, so that a read or write one byte outside is a
// report.  Exit status 0 unless the files cannot be read or written.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../vireo_amd/csrc/vrx_bgzf.h"

static bool put(FILE* f, const void* p, size_t n) { return n == 0 || fwrite(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: bgzf_host CASES RESULTS\n");
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) {
        fprintf(stderr, "bgzf_host: cannot open the files\n");
        return 2;
    }
    VrxBgzfWork* w = static_cast<VrxBgzfWork*>(malloc(sizeof(VrxBgzfWork)));
    if (!w) return 2;
    memset(w, 0, sizeof *w);
    vrx_bgzf_crc_init(w->crc);
    uint32_t n = 0;
    bool ok = true;
    while (ok && fread(&n, sizeof n, 1, in) == 1) {
        uint8_t* image = static_cast<uint8_t*>(malloc(n ? n : 1));
        if (!image || (n && fread(image, 1, n, in) != n)) return 2;
        int64_t count = 0;
        int32_t rc = vrx_bgzf_scan_image(image, n, 0, &count, nullptr, nullptr, nullptr, nullptr);
        std::vector<int64_t> off((size_t)count), start((size_t)count + 1);
        std::vector<int32_t> len((size_t)count), isize((size_t)count);
        int64_t again = 0;
        const int32_t rc2 = vrx_bgzf_scan_image(image, n, count, &again, off.data(), len.data(), isize.data(), start.data());
        if (rc2 != rc || again != count) return 3;
        const uint32_t members = (uint32_t)count;
        ok = put(out, &rc, sizeof rc) && put(out, &members, sizeof members);
        for (int64_t m = 0; ok && m < count; ++m) {
            const uint32_t pl = (uint32_t)len[(size_t)m], want = (uint32_t)isize[(size_t)m];
            uint8_t* payload = static_cast<uint8_t*>(malloc(pl ? pl : 1));
            uint8_t* text = static_cast<uint8_t*>(malloc(want ? want : 1));
            if (!payload || !text) return 2;
            memcpy(payload, image + off[(size_t)m], pl);
            const uint32_t crc = vrx_bgzf_le32(image + off[(size_t)m] + pl);
            const uint32_t st = vrx_bgzf_member(*w, payload, pl, want, crc, text);
            const uint32_t got = st ? 0 : want;
            ok = put(out, &st, sizeof st) && put(out, &got, sizeof got) && put(out, text, got);
            free(text);
            free(payload);
        }
        free(image);
    }
    free(w);
    fclose(in);
    if (fclose(out) != 0 || !ok) {
        fprintf(stderr, "bgzf_host: cannot write the results\n");
        return 2;
    }
    return 0;
}
