// tests/hostsim/sparse_pack_main.cpp -- TEST INFRASTRUCTURE: the sparse pack and the simulated load phase of jda_sparse_tiles over
// progressive files, as a program of its own so that it can be built with -fsanitize=address,undefined (tests/test_sparse_coef_cpu.py).
// For every file named on the command line: every scan decoded on the host, the sparse form packed, re-expanded and compared, and both
// load phases run over every tile (coefsparsesim_run).  Exit status 0: every file passed.
#include <stdint.h>
#include <stdio.h>

#include <vector>

extern "C" int coefsparsesim_run(const uint8_t *jpeg, int len, const int16_t *coefs, uint32_t n_blocks, int pixel_type, int options, const int32_t *rect,
                                 uint8_t *out, int pitch, int width_px, int rows, int32_t *info);

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s file.jpg ...\n", argv[0]); return 2; }
    int bad = 0;
    for (int a = 1; a < argc; a++) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "%s: cannot open\n", argv[a]); return 2; }
        std::vector<uint8_t> d;
        uint8_t buf[65536];
        size_t k;
        while ((k = fread(buf, 1, sizeof(buf), f)) > 0) d.insert(d.end(), buf, buf + k);
        fclose(f);
        int32_t info[3] = { 0, -1, 0 };
        const int rc = coefsparsesim_run(d.data(), (int)d.size(), NULL, 0, 0, 0, NULL, NULL, 0, 0, 0, info);
        printf("%s: rc %d, %d tiles, longest range %d\n", argv[a], rc, info[0], info[2]);
        if (rc != 0 || info[0] == 0) bad++;
    }
    return bad ? 1 : 0;
}
