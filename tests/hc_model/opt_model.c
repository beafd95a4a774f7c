/*
 * tests/hc_model/opt_model.c -- CPU model of the price-based optimal LZ4 block
 * parse of lz4m_compress_opt_batch (python-lz4_amd/csrc/lz4m_opt.hip), as
 * DESIGN.md section 9.7 defines it.  The HIP kernels must produce these bytes.
 * Plain C99, no dependency; the tests build it with gcc at run time.
 *
 * The parse, serially (n >= 13; shorter blocks are one literal run):
 *   tables    h(p) = (LE32(src + p) * 2654435761) >> (32 - 13); head[h] the
 *             newest inserted position with that hash, chain[p] the distance
 *             from p to the previous position with p's hash (0: none within
 *             65535 bytes) -- section 9.1's tables; attempts by the same level
 *             table (level < 1 -> 9, > 9 -> 9, 3 -> 4 ... 9 -> 256);
 *   matches   for every q <= n - 12, with every position below q inserted:
 *             walk the chain newest first for at most `attempts` candidates
 *             within 65535 bytes, each measured forwards only, up to lim =
 *             min(n - 5 - q, 65535) bytes; L[q] is the longest (>= 4), O[q]
 *             its distance, the first (nearest) among equals; the walk stops
 *             at a match of lim bytes.  Positions after n - 12 have none;
 *   prices    backwards from cost[n] = 1 (the last token), lit[n] = 0:
 *             cost[p] is the exact size of src[p..n) when a sequence starts at
 *             p, lit[p] that encoding's leading literal run.
 *             literal: l = lit[p + 1] + 1, cost[p + 1] + 1 + (l >= 15 and
 *             (l - 15) % 255 == 0);
 *             match: for ml = L[p] down to max(4, L[p] - 63): 3 +
 *             ext_bytes(ml - 4) + cost[p + ml]; the cheapest, the longest
 *             among equals; a match wins a tie with the literal (lit[p] = 0);
 *   emit      follow the choices from 0; the size is cost[0] (asserted);
 *   output    the block is written only if cost[0] <= cap; otherwise the
 *             result is 0 and dst is not touched.
 */
#include <assert.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define OPT_HASH_BITS 13
#define OPT_MAX_DIST 65535
#define OPT_LENGTHS 64   /* K: match lengths priced per position */

int opt_model_attempts(int level) {
    if (level < 1) level = 9;
    if (level > 9) level = 9;          /* deeper searches for levels 10-12 are not modelled */
    return level < 3 ? 2 : 1 << (level - 1);
}

static uint32_t le32(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

static uint32_t opt_hash(const uint8_t* p) { return (le32(p) * 2654435761u) >> (32 - OPT_HASH_BITS); }

static int32_t ext_bytes(int32_t v) { return v >= 15 ? 1 + (v - 15) / 255 : 0; }

static uint8_t* put_ext(uint8_t* op, int32_t v) {
    if (v >= 15) {
        v -= 15;
        for (; v >= 255; v -= 255) *op++ = 255;
        *op++ = (uint8_t)v;
    }
    return op;
}

/* L[q], O[q] for every q < n (0: no match) */
static void opt_matches(const uint8_t* src, int32_t n, int attempts, uint32_t* head, uint16_t* chain, uint16_t* L,
                        uint16_t* O) {
    const int32_t mflimit = n - 12;
    int32_t pl = 0, po = 0;   /* L and O of q - 1 */
    memset(L, 0, (size_t)n * sizeof(uint16_t));
    memset(O, 0, (size_t)n * sizeof(uint16_t));
    for (int32_t q = 0; q <= mflimit; ++q) {
        const int32_t lim = n - 5 - q < 65535 ? n - 5 - q : 65535;
        const uint32_t h = opt_hash(src + q);
        int32_t best = 0, off = 0;
        uint32_t cur = head[h];
        for (int left = attempts; left > 0 && cur != 0 && q - (int32_t)(cur - 1) <= OPT_MAX_DIST; --left) {
            const int32_t c = (int32_t)(cur - 1);
            /* the match of q - 1 at the same distance, less its first byte, is known to hold here */
            int32_t fwd = q - c == po && pl > 1 ? pl - 1 : 0;
            if (best >= 4 && src[c + best] != src[q + best]) {
                fwd = 0;   /* cannot beat the best so far (best < lim here): not measured */
            } else {
                while (fwd + 8 <= lim && memcmp(src + c + fwd, src + q + fwd, 8) == 0) fwd += 8;
                while (fwd < lim && src[c + fwd] == src[q + fwd]) ++fwd;
            }
            if (fwd >= 4 && fwd > best) {
                best = fwd;
                off = q - c;
                if (best == lim) break;   /* nothing longer exists */
            }
            const uint32_t d = chain[c];
            cur = d ? cur - d : 0;
        }
        L[q] = (uint16_t)best;
        O[q] = (uint16_t)off;
        pl = best;
        po = off;
        /* insert q */
        {
            const uint32_t prev = head[h];
            const uint32_t d = prev ? (uint32_t)q + 1u - prev : 0u;
            chain[q] = (uint16_t)(d > OPT_MAX_DIST ? 0u : d);
            head[h] = (uint32_t)q + 1u;
        }
    }
}

/* cost[0] of the model's parse, the choices in M (M[p]: the match length taken
 * at p, 0: a literal); L, O from opt_matches */
static int32_t opt_prices(int32_t n, const uint16_t* L, uint16_t* M, int32_t* cost) {
    int32_t lit = 0;
    cost[n] = 1;
    for (int32_t p = n - 1; p >= 0; --p) {
        const int32_t l = lit + 1;
        const int32_t lc = cost[p + 1] + 1 + (l >= 15 && (l - 15) % 255 == 0);
        int32_t mc = INT32_MAX, mlen = 0;
        if (L[p]) {
            const int32_t lo = L[p] - (OPT_LENGTHS - 1) > 4 ? L[p] - (OPT_LENGTHS - 1) : 4;
            for (int32_t ml = L[p]; ml >= lo; --ml) {
                const int32_t c = 3 + ext_bytes(ml - 4) + cost[p + ml];
                if (c < mc) {   /* the longest among equals */
                    mc = c;
                    mlen = ml;
                }
            }
        }
        if (mlen && mc <= lc) {
            cost[p] = mc;
            M[p] = (uint16_t)mlen;
            lit = 0;
        } else {
            cost[p] = lc;
            M[p] = 0;
            lit = l;
        }
    }
    return cost[0];
}

static uint8_t* opt_put_seq(uint8_t* o, const uint8_t* lits, int32_t ll, int32_t off, int32_t ml) {
    const int32_t mt = ml ? (ml - 4 < 15 ? ml - 4 : 15) : 0;
    *o++ = (uint8_t)(((ll < 15 ? ll : 15) << 4) | mt);
    o = put_ext(o, ll);
    if (ll) memcpy(o, lits, (size_t)ll);
    o += ll;
    if (ml) {
        *o++ = (uint8_t)(off & 0xFF);
        *o++ = (uint8_t)(off >> 8);
        o = put_ext(o, ml - 4);
    }
    return o;
}

/* the block's size (its cost[0]) without writing it; 0 on a bad argument */
static int opt_run(const uint8_t* src, int n, uint8_t* dst, int cap, int level, int write) {
    if (n < 0 || cap < 0 || n > 0x7E000000) return 0;
    if (n < 13) {
        const int size = 1 + n;   /* a token and n < 15 literals */
        if (!write) return size;
        if (size > cap) return 0;
        opt_put_seq(dst, src, n, 0, 0);
        return size;
    }
    uint32_t* head = (uint32_t*)calloc((size_t)1 << OPT_HASH_BITS, sizeof(uint32_t));
    uint16_t* chain = (uint16_t*)calloc((size_t)n, sizeof(uint16_t));
    uint16_t* L = (uint16_t*)malloc((size_t)n * sizeof(uint16_t));
    uint16_t* O = (uint16_t*)malloc((size_t)n * sizeof(uint16_t));
    uint16_t* M = (uint16_t*)malloc((size_t)n * sizeof(uint16_t));
    int32_t* cost = (int32_t*)malloc(((size_t)n + 1) * sizeof(int32_t));
    int size = 0;
    if (head && chain && L && O && M && cost) {
        opt_matches(src, n, opt_model_attempts(level), head, chain, L, O);
        size = opt_prices(n, L, M, cost);
        if (write && size > cap) size = 0;
        if (write && size) {
            uint8_t* o = dst;
            int32_t anchor = 0, p = 0;
            while (p < n) {
                if (M[p]) {
                    o = opt_put_seq(o, src + anchor, p - anchor, O[p], M[p]);
                    p += M[p];
                    anchor = p;
                } else {
                    ++p;
                }
            }
            o = opt_put_seq(o, src + anchor, n - anchor, 0, 0);
            assert(o - dst == size);
            if (o - dst != size) abort();
        }
    }
    free(head);
    free(chain);
    free(L);
    free(O);
    free(M);
    free(cost);
    return size;
}

int opt_model_compress(const uint8_t* src, int n, uint8_t* dst, int cap, int level) {
    return opt_run(src, n, dst, cap, level, 1);
}

/* cost[0] of the price pass alone (what opt_model_compress's size must equal) */
int opt_model_cost(const uint8_t* src, int n, int level) { return opt_run(src, n, NULL, 0, level, 0); }

/* A small safe decoder (the check program decodes the model's output with it):
 * returns the decoded size, or -1 on any malformed or overlong input. */
int opt_model_decode(const uint8_t* src, int n, uint8_t* dst, int cap) {
    int64_t ip = 0, op = 0;
    if (n <= 0) return -1;
    for (;;) {
        if (ip >= n) return -1;
        const uint32_t tok = src[ip++];
        int64_t ll = tok >> 4;
        if (ll == 15) {
            uint32_t b;
            do {
                if (ip >= n) return -1;
                b = src[ip++];
                ll += b;
            } while (b == 255);
        }
        if (ll > n - ip || ll > cap - op) return -1;
        if (ll) memcpy(dst + op, src + ip, (size_t)ll);
        ip += ll;
        op += ll;
        if (ip == n) return (tok & 15) ? -1 : (int)op;
        if (n - ip < 2) return -1;
        const int64_t off = (int64_t)src[ip] | ((int64_t)src[ip + 1] << 8);
        ip += 2;
        int64_t ml = tok & 15;
        if (ml == 15) {
            uint32_t b;
            do {
                if (ip >= n) return -1;
                b = src[ip++];
                ml += b;
            } while (b == 255);
        }
        ml += 4;
        if (off == 0 || off > op || ml > cap - op) return -1;
        for (int64_t k = 0; k < ml; ++k) dst[op + k] = dst[op + k - off];
        op += ml;
    }
}
