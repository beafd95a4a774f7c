/*
 * tests/hc_model/opt_model_check.c -- stand-alone check of opt_model.c, meant
 * to be built with -fsanitize=address,undefined (tests/test_opt_model.py
 * does) and run as its own process.  Every input is compressed by the model into an
 * exactly sized heap buffer (so a write past the capacity is caught), decoded
 * by the model's own safe decoder and compared; the exact-fit and the
 * one-byte-short capacities are checked too, and the size against the price
 * pass's cost[0].  Exit status 0 = all good.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int opt_model_compress(const uint8_t* src, int n, uint8_t* dst, int cap, int level);
int opt_model_decode(const uint8_t* src, int n, uint8_t* dst, int cap);
int opt_model_cost(const uint8_t* src, int n, int level);

static uint32_t rng_state = 12345u;
static uint32_t rng(void) {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

static int bound(int n) { return n + n / 255 + 16; }

static int failures = 0;

static void check(const char* what, const uint8_t* src, int n, int level) {
    const int cap = bound(n);
    uint8_t* dst = (uint8_t*)malloc((size_t)cap);
    uint8_t* back = (uint8_t*)malloc((size_t)n + 1);
    const int r = opt_model_compress(src, n, dst, cap, level);
    if (r <= 0 || r > cap || r != opt_model_cost(src, n, level)) {
        printf("FAIL %s n=%d level=%d: size %d\n", what, n, level, r);
        ++failures;
    } else {
        const int d = opt_model_decode(dst, r, back, n);
        if (d != n || memcmp(back, src, (size_t)n) != 0) {
            printf("FAIL %s n=%d level=%d: decodes to %d bytes or differs\n", what, n, level, d);
            ++failures;
        }
        /* exact fit: same bytes; one byte short: 0 */
        uint8_t* tight = (uint8_t*)malloc((size_t)r);
        const int r2 = opt_model_compress(src, n, tight, r, level);
        if (r2 != r || memcmp(tight, dst, (size_t)r) != 0) {
            printf("FAIL %s n=%d level=%d: exact capacity gives %d, not %d\n", what, n, level, r2, r);
            ++failures;
        }
        free(tight);
        tight = (uint8_t*)malloc((size_t)r);   /* r - 1 usable bytes, the last one a sentinel */
        tight[r - 1] = 0xA5;
        if (opt_model_compress(src, n, tight, r - 1, level) != 0 || tight[r - 1] != 0xA5) {
            printf("FAIL %s n=%d level=%d: capacity %d not refused cleanly\n", what, n, level, r - 1);
            ++failures;
        }
        free(tight);
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

int main(void) {
    static const int lens[] = {0, 1, 4, 5, 11, 12, 13, 14, 16, 17, 64, 65535, 65536, 65537, 200003};
    static const int kinds[] = {0, 1, 2, 3, 4, 7, 8, 9};
    static const int levels[] = {3, 9};
    uint8_t* buf = (uint8_t*)malloc(3 * 65537 + 1000);
    for (unsigned li = 0; li < sizeof lens / sizeof *lens; ++li)
        for (unsigned ki = 0; ki < sizeof kinds / sizeof *kinds; ++ki)
            for (unsigned vi = 0; vi < sizeof levels / sizeof *levels; ++vi) {
                const int n = lens[li];
                /* every position is searched and priced here, not only the parse's, and every input is
                 * compressed four times: the long inputs at 4 attempts only, as zeros, random bytes and
                 * text (the longest as zeros and text); the buffers' bounds depend on neither */
                if (n > 64 && levels[vi] > 3) continue;
                if (n > 64 && kinds[ki] != 0 && kinds[ki] != 8 && kinds[ki] != 9) continue;
                if (n > 65537 && kinds[ki] == 8) continue;
                uint8_t* exact = (uint8_t*)malloc((size_t)n + 1);   /* reads past n are caught */
                fill(exact, n, kinds[ki]);
                check("fill", exact, n, levels[vi]);
                free(exact);
            }
    memset(buf, 0, 70000);
    check("zeros70000", buf, 70000, 9);
    for (int period = 65535; period <= 65537; ++period) {   /* the window's edge */
        const int n = 3 * period + 1000;
        for (int i = 0; i < period; ++i) buf[i] = (uint8_t)rng();
        for (int i = period; i < n; ++i) buf[i] = buf[i - period];
        uint8_t* exact = (uint8_t*)malloc((size_t)n);
        memcpy(exact, buf, (size_t)n);
        check("period", exact, n, 4);
        free(exact);
    }
    free(buf);
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("opt_model_check: ok\n");
    return 0;
}
