// Stand-alone host check of csrc/jpeg_encode.h: every case of a manifest is built into a whole JPEG file from the shared per-block
// functions, called block after block, and compared with the bytes the NumPy restatement (tests/jpeg_encode_scenario.py) gave.
// Built with -fsanitize=address,undefined by tests/test_jpeg_encode_scenario_host.py and run as its own process.
//   manifest line: <pixels file> <expected file> H W C quality sampling
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "jpeg_encode.h"

static const JpeTables kTables = jpe_make_tables();

static std::vector<uint8_t> read_file(const char* path) {
    std::vector<uint8_t> out;
    FILE* f = fopen(path, "rb");
    if (!f) return out;
    uint8_t buf[4096];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
    fclose(f);
    return out;
}

struct HostOr {
    uint32_t* words;
    void operator()(uint32_t i, uint32_t v) const { words[i] |= v; }
};

static std::vector<uint8_t> encode(const uint8_t* px, int H, int W, int C, int quality, int sampling) {
    const JpeGeometry g = jpe_geometry(H, W, C, sampling);
    std::vector<int16_t> zz((size_t)g.nblk * 64);
    std::vector<int> nbits(g.nblk);
    // blocks: samples, DCT, quantisation, zig-zag; a dummy repeats its source's DC
    for (int i = 0; i < g.nblk; ++i) {
        const JpeBlock b = jpe_block(g, i);
        int16_t* out = &zz[(size_t)i * 64];
        if (b.source != i) {
            for (int k = 0; k < 64; ++k) out[k] = 0;
            out[0] = zz[(size_t)b.source * 64];
            continue;
        }
        int d[64];
        for (int y = 0; y < 8; ++y)
            for (int x = 0; x < 8; ++x) d[8 * y + x] = jpe_sample(px, g, b.comp, 8 * b.bx + x, 8 * b.by + y) - 128;
        jpe_fdct(d);
        const int t = b.comp ? 1 : 0;
        for (int k = 0; k < 64; ++k) out[k] = (int16_t)jpe_quantise(d[kTables.natural[k]], jpe_quant(kTables.base[t][kTables.natural[k]], quality));
    }
    // bit counts and offsets
    uint64_t total = 0;
    std::vector<uint64_t> offset(g.nblk);
    for (int i = 0; i < g.nblk; ++i) {
        const JpeBlock b = jpe_block(g, i);
        const int t = b.comp ? 1 : 0;
        const int diff = zz[(size_t)i * 64] - (b.pred >= 0 ? zz[(size_t)b.pred * 64] : 0);
        nbits[i] = jpe_dc_bits(kTables, t, diff) + jpe_ac_bits(kTables, t, &zz[(size_t)i * 64]);
        if (nbits[i] > JPE_MAX_BLOCK_BITS) { fprintf(stderr, "a block of %d bits\n", nbits[i]); exit(2); }
        offset[i] = total;
        total += nbits[i];
    }
    // bits
    std::vector<uint32_t> words(total / 32 + 2, 0u);
    for (int i = 0; i < g.nblk; ++i) {
        const JpeBlock b = jpe_block(g, i);
        const int diff = zz[(size_t)i * 64] - (b.pred >= 0 ? zz[(size_t)b.pred * 64] : 0);
        JpeWordSink<HostOr> sink{HostOr{words.data()}, (uint32_t)offset[i]};
        jpe_block_bits(kTables, b.comp ? 1 : 0, &zz[(size_t)i * 64], diff, sink);
        if (sink.pos != (uint32_t)(offset[i] + nbits[i])) { fprintf(stderr, "block %d: counted %d bits, wrote %u\n", i, nbits[i], sink.pos - (uint32_t)offset[i]); exit(2); }
    }
    const int pad = (int)((8 - total % 8) % 8);
    if (pad) {
        JpeWordSink<HostOr> sink{HostOr{words.data()}, (uint32_t)total};
        sink.put((1u << pad) - 1, pad);
    }
    const size_t nraw = (size_t)((total + 7) / 8);
    std::vector<uint8_t> raw(nraw);
    for (size_t j = 0; j < nraw; ++j) raw[j] = (uint8_t)(words[j >> 2] >> (24 - 8 * (j & 3)));
    // file
    std::vector<uint8_t> file(JPE_MAX_HEADER);
    const int nh = jpe_header(kTables, file.data(), H, W, C, quality, sampling);
    if (nh != jpe_header_bytes(C)) { fprintf(stderr, "header of %d bytes, jpe_header_bytes says %d\n", nh, jpe_header_bytes(C)); exit(2); }
    file.resize(nh + 2 * nraw + 2);
    const int64_t ns = jpe_stuff(raw.data(), (int64_t)nraw, file.data() + nh);
    file[nh + ns] = 0xFF;
    file[nh + ns + 1] = 0xD9;
    file.resize(nh + ns + 2);
    if ((int64_t)file.size() > jpe_bound(H, W, C, sampling)) { fprintf(stderr, "a file of %zu bytes above the bound %lld\n", file.size(), (long long)jpe_bound(H, W, C, sampling)); exit(2); }
    return file;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s manifest\n", argv[0]); return 2; }
    FILE* m = fopen(argv[1], "r");
    if (!m) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    char pixels[1024], expected[1024];
    int H, W, C, quality, sampling, files = 0, failures = 0;
    while (fscanf(m, "%1023s %1023s %d %d %d %d %d", pixels, expected, &H, &W, &C, &quality, &sampling) == 7) {
        const std::vector<uint8_t> px = read_file(pixels), want = read_file(expected);
        if (px.size() != (size_t)H * W * C || want.empty()) { fprintf(stderr, "%s: unreadable\n", pixels); return 2; }
        const std::vector<uint8_t> got = encode(px.data(), H, W, C, quality, sampling);
        ++files;
        if (got != want) {
            size_t at = 0;
            while (at < got.size() && at < want.size() && got[at] == want[at]) ++at;
            printf("MISMATCH %s: %zu bytes against %zu, first difference at %zu\n", expected, got.size(), want.size(), at);
            ++failures;
        }
    }
    fclose(m);
    printf("files %d failures %d\n", files, failures);
    return failures ? 1 : 0;
}
