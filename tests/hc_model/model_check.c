/*
 * tests/hc_model/model_check.c -- stand-alone check of the three CPU models
 * (hc_model.c: HC and HC with a prefix; opt_model.c, which includes it), meant
 * to be built with -fsanitize=address,undefined (hc_support.check_program
 * does) and run as its own process.  Prefix and block sit in one exactly sized
 * heap buffer (a read before the prefix or past the block is caught), the
 * model compresses into an exactly sized buffer (so is a write past the
 * capacity), the result is decoded by the models' own safe decoder with the
 * prefix as its dictionary and compared; the exact-fit and one-byte-short
 * capacities are checked too, the optimal parse's size against the price
 * pass's cost[0], and a prefix of 0 bytes must give hc_model_compress's bytes.
 * One "<model>_check: ok" line per model; exit status 0 = all good.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int hc_model_compress(const uint8_t* src, int n, uint8_t* dst, int cap, int level);
int hc_model_compress_prefix(const uint8_t* base, int prefix_len, int n, uint8_t* dst, int cap, int level);
int hc_model_decode_prefix(const uint8_t* src, int n, const uint8_t* dict, int dict_len, uint8_t* dst, int cap);
int opt_model_compress(const uint8_t* src, int n, uint8_t* dst, int cap, int level);
int opt_model_cost(const uint8_t* src, int n, int level);

/* a model as check() sees it: the block is the n bytes at base + P */
typedef int (*compress_fn)(const uint8_t* base, int P, int n, uint8_t* dst, int cap, int level);

static int hc_plain(const uint8_t* base, int P, int n, uint8_t* dst, int cap, int level) {
    return P == 0 ? hc_model_compress(base, n, dst, cap, level) : -1;
}
static int opt_plain(const uint8_t* base, int P, int n, uint8_t* dst, int cap, int level) {
    return P == 0 ? opt_model_compress(base, n, dst, cap, level) : -1;
}

static uint32_t rng_state;
static uint32_t rng(void) {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

static int bound(int n) { return n + n / 255 + 16; }

static int failures = 0;

/* base: exactly P + n heap bytes */
static void check(compress_fn compress, const char* what, const uint8_t* base, int P, int n, int level) {
    const int cap = bound(n);
    uint8_t* dst = (uint8_t*)malloc((size_t)cap);
    uint8_t* back = (uint8_t*)malloc((size_t)n + 1);
    const int r = compress(base, P, n, dst, cap, level);
    if (r <= 0 || r > cap || (compress == opt_plain && r != opt_model_cost(base, n, level))) {
        printf("FAIL %s P=%d n=%d level=%d: size %d\n", what, P, n, level, r);
        ++failures;
    } else {
        const int d = hc_model_decode_prefix(dst, r, base, P, back, n);
        if (d != n || memcmp(back, base + P, (size_t)n) != 0) {
            printf("FAIL %s P=%d n=%d level=%d: decodes to %d bytes or differs\n", what, P, n, level, d);
            ++failures;
        }
        /* exact fit: same bytes; one byte short: 0 */
        uint8_t* tight = (uint8_t*)malloc((size_t)r);
        const int r2 = compress(base, P, n, tight, r, level);
        if (r2 != r || memcmp(tight, dst, (size_t)r) != 0) {
            printf("FAIL %s P=%d n=%d level=%d: exact capacity gives %d, not %d\n", what, P, n, level, r2, r);
            ++failures;
        }
        free(tight);
        tight = (uint8_t*)malloc((size_t)r);   /* r - 1 usable bytes, the last one a sentinel */
        tight[r - 1] = 0xA5;
        if (compress(base, P, n, tight, r - 1, level) != 0 || tight[r - 1] != 0xA5) {
            printf("FAIL %s P=%d n=%d level=%d: capacity %d not refused cleanly\n", what, P, n, level, r - 1);
            ++failures;
        }
        free(tight);
        if (compress == hc_model_compress_prefix && P == 0) {
            uint8_t* plain = (uint8_t*)malloc((size_t)cap);
            const int r3 = hc_model_compress(base, n, plain, cap, level);
            if (r3 != r || memcmp(plain, dst, (size_t)r) != 0) {
                printf("FAIL %s n=%d level=%d: an empty prefix changes the bytes\n", what, n, level);
                ++failures;
            }
            free(plain);
        }
    }
    free(dst);
    free(back);
}

static void fill(uint8_t* buf, int n, int kind) {
    static const char* words[] = {"the ", "of ", "and ", "block ", "compress ", "wave ", "lane ", "chain ",
                                  "hash ", "match ", "literal ", "offset ", "a ", "in ", "to ", "kernel "};
    int i = 0;
    switch (kind) {
        case 0: memset(buf, 0, (size_t)n); break;
        case 1: case 2: case 3: case 4: case 7:
            for (i = 0; i < n; ++i) buf[i] = (uint8_t)(0x41 + i % kind);
            break;
        case 8:
            for (i = 0; i < n; ++i) buf[i] = (uint8_t)rng();
            break;
        default:   /* word text */
            while (i < n) {
                const char* w = words[rng() % 16];
                for (; *w && i < n; ++w) buf[i++] = (uint8_t)*w;
            }
    }
}

/* The cases of a model without a prefix.  thin (the optimal parse: every
 * position is searched and priced, not only the parse's, and every input is
 * compressed four times): the long inputs at 4 attempts only, as zeros, random
 * bytes and text (the longest as zeros and text); the buffers' bounds depend
 * on neither. */
static void check_plain(compress_fn compress, int thin) {
    static const int lens[] = {0, 1, 4, 5, 11, 12, 13, 14, 16, 17, 64, 65535, 65536, 65537, 200003};
    static const int kinds[] = {0, 1, 2, 3, 4, 7, 8, 9};
    static const int levels[] = {3, 9};
    uint8_t* buf = (uint8_t*)malloc(3 * 65537 + 1000);
    rng_state = 12345u;
    for (unsigned li = 0; li < sizeof lens / sizeof *lens; ++li)
        for (unsigned ki = 0; ki < sizeof kinds / sizeof *kinds; ++ki)
            for (unsigned vi = 0; vi < sizeof levels / sizeof *levels; ++vi) {
                const int n = lens[li];
                if (thin && n > 64 && levels[vi] > 3) continue;
                if (thin && n > 64 && kinds[ki] != 0 && kinds[ki] != 8 && kinds[ki] != 9) continue;
                if (thin && n > 65537 && kinds[ki] == 8) continue;
                uint8_t* exact = (uint8_t*)malloc((size_t)n + 1);   /* reads past n are caught */
                fill(exact, n, kinds[ki]);
                check(compress, "fill", exact, 0, n, levels[vi]);
                free(exact);
            }
    memset(buf, 0, 70000);
    check(compress, "zeros70000", buf, 0, 70000, 9);
    for (int period = 65535; period <= 65537; ++period) {   /* the window's edge */
        const int n = 3 * period + 1000;
        for (int i = 0; i < period; ++i) buf[i] = (uint8_t)rng();
        for (int i = period; i < n; ++i) buf[i] = buf[i - period];
        uint8_t* exact = (uint8_t*)malloc((size_t)n);
        memcpy(exact, buf, (size_t)n);
        check(compress, "period", exact, 0, n, 4);
        free(exact);
    }
    free(buf);
}

static void check_prefix(void) {
    static const int plens[] = {0, 1, 3, 4, 7, 8, 63, 64, 65, 4096, 65535, 65536};
    static const int lens[] = {0, 1, 12, 13, 14, 64, 65, 4096, 65536, 65537};
    static const int kinds[] = {0, 1, 2, 3, 7, 8, 9};
    const compress_fn compress = hc_model_compress_prefix;
    rng_state = 54321u;
    for (unsigned pi = 0; pi < sizeof plens / sizeof *plens; ++pi)
        for (unsigned li = 0; li < sizeof lens / sizeof *lens; ++li)
            for (unsigned ki = 0; ki < sizeof kinds / sizeof *kinds; ++ki) {
                const int P = plens[pi], n = lens[li];
                uint8_t* base = (uint8_t*)malloc((size_t)P + (size_t)n + (P + n == 0));
                fill(base, P + n, kinds[ki]);   /* the pattern continues across the boundary */
                check(compress, "fill", base, P, n, (pi + li + ki) % 2 ? 3 : 9);
                free(base);
            }
    for (int shift = 0; shift <= 1; ++shift) {   /* the window's edge: distance 65535 is within reach, 65536 is not */
        const int P = 65536, n = 5000;
        uint8_t* base = (uint8_t*)malloc((size_t)P + n);
        fill(base, P, 8);
        memcpy(base + P, base + shift, 1000);
        fill(base + P + 1000, n - 1000, 8);
        check(compress, "edge", base, P, n, 4);
        free(base);
    }
    {   /* a run that crosses the boundary; a short block after a matching prefix */
        uint8_t* base = (uint8_t*)malloc(300 + 1000);
        memset(base, 0x5A, 1300);
        check(compress, "run", base, 300, 1000, 9);
        check(compress, "short", base, 300, 12, 9);
        free(base);
    }
}

/* one model's cases, then its line: ok only if they added no failure */
static void report(const char* name, int before) {
    if (failures == before) printf("%s_check: ok\n", name);
}

int main(void) {
    int before = failures;
    check_plain(hc_plain, 0);
    report("hc_model", before);
    before = failures;
    check_prefix();
    report("hc_model_prefix", before);
    before = failures;
    check_plain(opt_plain, 1);
    report("opt_model", before);
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    return 0;
}
