// Stand-alone host check of csrc/jpeg_decode.h (tests/test_jpeg_scenario_host.py builds it with -fsanitize=address,undefined and runs
// it as a child process; nothing here touches a GPU).  The parser, the bit reader, the symbol decode and the block step are the
// library's own source; this file adds a sequential driver around them.
//
//   jpeg_host_check MANIFEST        lines "path checksum-hex corruptions seed"
//
// Per file: parse, decode every restart interval sequentially, compare the coefficient checksum (tests/jpeg_scenario.py:
// coefficient_checksum) -- then `corruptions` seeded damaged copies (cuts inside the entropy-coded bytes, byte flips there): each must
// parse or be refused, decode to the end with every access inside its buffers, and a cut of 16 bytes or more must give a status.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "jpeg_decode.h"

static uint64_t rng_state;
static uint32_t rng() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

struct Decoded {
    int status;
    uint64_t checksum;
};

static Decoded decode(const std::vector<uint8_t>& file, const hps_jpeg_header& H) {
    static const uint8_t natural[64] = JPG_NATURAL_ORDER;
    const JpgGeometry g = jpg_geometry(H.width, H.height, H.ncomp, H.hs, H.vs, H.restart_interval);
    // the stuffing and the markers out, the interval starts recorded -- exactly sized buffers, so that the sanitizer sees every overrun
    std::vector<uint8_t> bytes;
    std::vector<uint32_t> istart(1, 0);
    int status = 0;
    for (int64_t i = 0; i < H.scan_length; ++i) {
        const uint8_t c = file[(size_t)H.scan_offset + i];
        const int next = i + 1 < H.scan_length ? file[(size_t)H.scan_offset + i + 1] : -1;
        if (c == 0xff && next == 0) {
            bytes.push_back(0xff);
            ++i;
        } else if (c == 0xff && next >= 0xd0 && next <= 0xd7) {
            if ((int)istart.size() < g.num_intervals && (next & 7) == (int)((istart.size() - 1) & 7)) {
                istart.push_back((uint32_t)bytes.size());
            } else {
                status |= HPS_JPEG_ST_MARKERS;
                if ((int)istart.size() < g.num_intervals) istart.push_back((uint32_t)bytes.size());
            }
            ++i;
        } else {
            bytes.push_back(c);
        }
    }
    while ((int)istart.size() <= g.num_intervals) istart.push_back((uint32_t)bytes.size());
    std::vector<uint32_t> words((bytes.size() + 3) / 4, 0);
    if (!bytes.empty()) memcpy(words.data(), bytes.data(), bytes.size());
    const JpgStream stream = {words.data(), (uint32_t)words.size()};

    std::vector<JpgTable> tabs(6);
    for (int t = 0; t < 6; ++t) {
        const hps_jpeg_huff* h = t < 3 ? &H.dc[t] : &H.ac[t - 3];
        memcpy(tabs[t].vals, h->vals, 256);
        jpg_table_lengths(h, &tabs[t]);
        for (int i = 0; i < (1 << JPG_LOOK_BITS); ++i) tabs[t].look[i] = jpg_look_entry(&tabs[t], i);
    }
    std::vector<int16_t> coefs((size_t)g.num_blocks * 64, 0);
    const int mcus = g.mcus_x * g.mcus_y;
    for (int k = 0; k < g.num_intervals; ++k) {
        const uint32_t iend = istart[k + 1] * 8u;
        const int last_mcu = (k + 1) * g.mcus_per_interval < mcus ? (k + 1) * g.mcus_per_interval : mcus;
        const uint32_t base = (uint32_t)(k * g.mcus_per_interval * g.bpm), limit = (uint32_t)(last_mcu * g.bpm) - base;
        JpgState st = {istart[k] * 8u, 0, 0, 0};
        JpgReader rd;
        jpg_reader_init(&rd, stream, st.p, iend);
        int pred[3] = {0, 0, 0};
        while (st.nblk < limit && st.p < iend) {
            const uint32_t comp = st.blk < (uint32_t)g.nluma ? 0u : st.blk - g.nluma + 1u, blk = base + st.nblk;
            int kout = 0, val = 0;
            const int fl = jpg_step(tabs.data(), g.nluma, g.bpm, &rd, &st, &kout, &val);
            if (fl & JPG_STEP_VALUE) {
                if (kout == 0) {
                    pred[comp] += val;
                    val = pred[comp];
                }
                coefs[(size_t)blk * 64 + natural[kout]] = (int16_t)val;
            }
            if (fl & JPG_STEP_ERROR) status |= HPS_JPEG_ST_CODE;
            if (st.p > iend) status |= HPS_JPEG_ST_OVERRUN;
        }
        if (st.nblk < limit) status |= HPS_JPEG_ST_SHORT;
    }
    uint64_t sum = 0;
    for (size_t i = 0; i < coefs.size(); ++i)
        sum += (uint64_t)(int64_t)coefs[i] * ((((uint64_t)i * 2654435761ull) & 0xffffffffull) | 1ull);
    return {status, sum};
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: jpeg_host_check MANIFEST\n");
        return 2;
    }
    FILE* mf = fopen(argv[1], "r");
    if (!mf) {
        fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    char path[1024];
    unsigned long long want;
    int corruptions;
    unsigned long long seed;
    int files = 0, failures = 0, damaged = 0, refused = 0, flagged = 0;
    while (fscanf(mf, "%1023s %llx %d %llu", path, &want, &corruptions, &seed) == 4) {
        FILE* f = fopen(path, "rb");
        if (!f) {
            fprintf(stderr, "cannot open %s\n", path);
            return 2;
        }
        std::vector<uint8_t> file;
        uint8_t buf[65536];
        size_t got;
        while ((got = fread(buf, 1, sizeof(buf), f)) > 0) file.insert(file.end(), buf, buf + got);
        fclose(f);
        ++files;
        hps_jpeg_header H;
        char msg[400];
        if (jpg_parse(file.data(), (int64_t)file.size(), &H, msg, sizeof(msg)) != 0) {
            printf("FAIL %s: parse: %s\n", path, msg);
            ++failures;
            continue;
        }
        const Decoded d = decode(file, H);
        if (d.status != 0 || d.checksum != want) {
            printf("FAIL %s: status %d, checksum %016llx, expected %016llx\n", path, d.status, (unsigned long long)d.checksum, want);
            ++failures;
        }
        rng_state = seed * 0x9e3779b97f4a7c15ull + 1;
        for (int c = 0; c < corruptions && H.scan_length > 0; ++c) {
            std::vector<uint8_t> bad(file);                       // a fresh exactly sized copy
            const bool cut = (c & 1) == 0;
            size_t removed = 0;
            if (cut) {
                const size_t keep = (size_t)H.scan_offset + rng() % (uint32_t)H.scan_length;
                removed = bad.size() - keep;
                bad.resize(keep);
                bad.shrink_to_fit();
            } else {
                for (int n = 1 + (int)(rng() % 3); n > 0; --n) bad[(size_t)H.scan_offset + rng() % (uint32_t)H.scan_length] ^= (uint8_t)(1 + rng() % 255);
            }
            ++damaged;
            hps_jpeg_header HB;
            if (jpg_parse(bad.data(), (int64_t)bad.size(), &HB, msg, sizeof(msg)) != 0) {
                ++refused;
                continue;
            }
            const Decoded b = decode(bad, HB);
            flagged += b.status != 0;
            if (cut && removed >= 16 + 2 && b.status == 0) {
                printf("FAIL %s: cut of %zu bytes decoded with status 0\n", path, removed);
                ++failures;
            }
        }
    }
    fclose(mf);
    printf("files %d damaged %d refused %d flagged %d failures %d\n", files, damaged, refused, flagged, failures);
    return failures ? 1 : 0;
}
