// Host half of the split JPEG decode (jpeg.h): marker parsing and Huffman decoding of baseline
// sequential frames — Motion-JPEG AVI frames and the reference's frame<N>.jpg directories
// (utils.py:851-860) — into per-block offsets and the non-zero quantised coefficients; the
// pixels are reconstructed on the device (jpeg_recon.hip).  Plain C++, no device memory.
//
// Everything outside baseline YCbCr / grayscale with 4:4:4, 4:2:2 or 4:2:0 sampling in one
// interleaved scan is reported as unsupported (the caller decodes such frames with libjpeg), a
// malformed or truncated stream is an error; no read goes past the frame's bytes.
#include <cstring>

#include "jpeg.h"
#include "mvp_common.h"

namespace jpeg {
namespace {

const uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                              41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                              30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ITU-T T.81 Annex K.3 typical Huffman tables: what a frame without DHT segments means
// (Motion-JPEG's habit; libjpeg-turbo installs them in every slot 0 / 1 left undefined)
const uint8_t kDcLumBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
const uint8_t kDcChrBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kAcLumBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
const uint8_t kAcLumVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
    0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
    0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
const uint8_t kAcChrBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
const uint8_t kAcChrVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
    0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
    0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
    0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
    0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

constexpr int LOOK = 10;  // bits of the one-step lookup

struct Huff {
    bool defined = false;
    uint16_t look[1 << LOOK];  // length << 8 | symbol for codes of <= LOOK bits, 0 = longer
    int32_t maxcode[18];       // largest code of each length (-1: none), left-aligned compare
    int32_t valoff[17];
    uint8_t vals[256];

    // bits[l - 1] codes of length l, symbols in code order (T.81 Annex C); false if the counts
    // do not describe a prefix code
    bool build(const uint8_t* bits, const uint8_t* symbols, int n_sym) {
        std::memset(look, 0, sizeof(look));
        std::memcpy(vals, symbols, (size_t)n_sym);
        int code = 0, k = 0;
        for (int l = 1; l <= 16; l++) {
            valoff[l] = k - code;
            for (int i = 0; i < bits[l - 1]; i++, k++, code++) {
                if (code >= (1 << l)) return false;
                if (l <= LOOK) {
                    const int lo = code << (LOOK - l);
                    for (int j = 0; j < (1 << (LOOK - l)); j++) look[lo + j] = (uint16_t)(l << 8 | symbols[k]);
                }
            }
            maxcode[l] = bits[l - 1] ? code - 1 : -1;
            code <<= 1;
        }
        maxcode[17] = 0x7fffffff;
        defined = true;
        return true;
    }
};

const Huff& standard_table(int cls, int slot) {
    static const struct Std {
        Huff t[2][2];
        Std() {
            t[0][0].build(kDcLumBits, kDcVals, 12);
            t[0][1].build(kDcChrBits, kDcVals, 12);
            t[1][0].build(kAcLumBits, kAcLumVals, 162);
            t[1][1].build(kAcChrBits, kAcChrVals, 162);
        }
    } std_tables;
    return std_tables.t[cls][slot];
}

struct Header {
    mvp_jpeg_frame_info info{};
    uint16_t qt[4][64];
    bool qt_seen[4] = {false, false, false, false};
    Huff huff[2][4];            // [class: 0 DC, 1 AC][slot]
    int comp_id[4] = {0, 0, 0, 0}, comp_h[4] = {0, 0, 0, 0}, comp_v[4] = {0, 0, 0, 0}, comp_tq[4] = {0, 0, 0, 0};
    int comp_td[3] = {0, 0, 0}, comp_ta[3] = {0, 0, 0};
    int restart = 0;
    bool jfif = false, adobe = false, sof = false;
    size_t scan = 0;            // first byte of the entropy-coded data
};

[[noreturn]] void bad(const char* what, size_t at) { mvp::fail(MVP_ERR_ARG, "jpeg: %s at byte %zu", what, at); }

void unsupported(Header& h, int why) {
    if (h.info.status == MVP_JPEG_OK) h.info.status = why;
}

// Walks the markers up to and including the SOS header.  Throws on a malformed / truncated
// stream; an unsupported kind of frame sets info.status (the first reason met) and parsing goes on
// only as far as needed to report the frame's size.
void parse_header(const uint8_t* d, size_t n, Header& h) {
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) bad("no SOI marker", 0);
    size_t p = 2;
    for (;;) {
        if (p >= n) bad("truncated before the scan", p);
        if (d[p] != 0xFF) bad("marker expected", p);
        while (p < n && d[p] == 0xFF) p++;  // fill bytes
        if (p >= n) bad("truncated before the scan", p);
        const int m = d[p++];
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;  // TEM, stray RSTn: no payload
        if (m == 0xD8) bad("second SOI", p - 2);
        if (m == 0xD9) bad("EOI before any scan", p - 2);
        if (m == 0x00) bad("marker expected", p - 2);
        if (p + 2 > n) bad("truncated segment", p);
        const size_t len = (size_t)d[p] << 8 | d[p + 1];
        if (len < 2 || p + len > n) bad("truncated segment", p);
        const uint8_t* s = d + p + 2;
        const size_t sl = len - 2;
        const size_t seg = p;
        p += len;
        if (m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {  // SOFn
            if (h.sof) bad("second frame header", seg);
            if (sl < 6) bad("short frame header", seg);
            h.sof = true;
            const int prec = s[0], nf = s[5];
            h.info.height = s[1] << 8 | s[2];
            h.info.width = s[3] << 8 | s[4];
            h.info.components = nf;
            if (sl != (size_t)6 + 3 * nf) bad("frame header length", seg);
            if (h.info.width == 0 || h.info.height == 0) bad("empty frame", seg);
            if (m != 0xC0) unsupported(h, MVP_JPEG_PROCESS);
            if (prec != 8) unsupported(h, MVP_JPEG_PRECISION);
            if (nf != 1 && nf != 3) unsupported(h, MVP_JPEG_COMPONENTS);
            for (int c = 0; c < nf && c < 4; c++) {
                h.comp_id[c] = s[6 + 3 * c];
                h.comp_h[c] = s[7 + 3 * c] >> 4;
                h.comp_v[c] = s[7 + 3 * c] & 15;
                h.comp_tq[c] = s[8 + 3 * c];
                if (h.comp_tq[c] > 3) bad("quantisation table number", seg);
            }
            if (nf == 1 || nf == 3) {
                const int hs = h.comp_h[0], vs = h.comp_v[0];
                bool ok = nf == 1 ? (hs == 1 && vs == 1)
                                  : ((hs == 1 || hs == 2) && (vs == 1 || (vs == 2 && hs == 2)) && h.comp_h[1] == 1 &&
                                     h.comp_v[1] == 1 && h.comp_h[2] == 1 && h.comp_v[2] == 1);
                if (!ok) unsupported(h, MVP_JPEG_SAMPLING);
                h.info.h_samp = hs;
                h.info.v_samp = vs;
            }
        } else if (m == 0xCC) {
            unsupported(h, MVP_JPEG_PROCESS);  // arithmetic conditioning
        } else if (m == 0xDB) {                // DQT
            size_t q = 0;
            while (q < sl) {
                const int pq = s[q] >> 4, tq = s[q] & 15;
                if (tq > 3 || pq > 1) bad("quantisation table header", seg);
                const size_t need = pq ? 128 : 64;
                if (q + 1 + need > sl) bad("short quantisation table", seg);
                if (pq) {
                    unsupported(h, MVP_JPEG_PRECISION);
                } else {
                    for (int i = 0; i < 64; i++) h.qt[tq][kNatural[i]] = s[q + 1 + i];
                    h.qt_seen[tq] = true;
                }
                q += 1 + need;
            }
        } else if (m == 0xC4) {                // DHT
            size_t q = 0;
            while (q < sl) {
                if (q + 17 > sl) bad("short Huffman table", seg);
                const int tc = s[q] >> 4, th = s[q] & 15;
                if (tc > 1 || th > 3) bad("Huffman table header", seg);
                int cnt = 0;
                for (int i = 0; i < 16; i++) cnt += s[q + 1 + i];
                if (cnt > 256 || q + 17 + cnt > sl) bad("short Huffman table", seg);
                if (!h.huff[tc][th].build(s + q + 1, s + q + 17, cnt)) bad("Huffman table is no prefix code", seg);
                q += 17 + (size_t)cnt;
            }
        } else if (m == 0xDD) {                // DRI
            if (sl != 2) bad("restart interval length", seg);
            h.restart = s[0] << 8 | s[1];
        } else if (m == 0xE0) {
            if (sl >= 14 && !std::memcmp(s, "JFIF\0", 5)) h.jfif = true;
        } else if (m == 0xEE) {
            if (sl >= 12 && !std::memcmp(s, "Adobe", 5)) h.adobe = true;
        } else if (m == 0xDC) {
            unsupported(h, MVP_JPEG_PROCESS);  // DNL: the height comes after the scan
        } else if (m == 0xDA) {                // SOS
            if (!h.sof) bad("scan before the frame header", seg);
            if (h.info.status != MVP_JPEG_OK) return;
            const int nc = h.info.components;
            if (sl < 1) bad("short scan header", seg);
            const int ns = s[0];
            if (ns < 1 || ns > 4 || sl != (size_t)4 + 2 * ns) bad("scan header length", seg);
            if (ns != nc) return unsupported(h, MVP_JPEG_SCANS);
            for (int c = 0; c < nc; c++) {
                if (s[1 + 2 * c] != h.comp_id[c]) return unsupported(h, MVP_JPEG_SCANS);
                h.comp_td[c] = s[2 + 2 * c] >> 4;
                h.comp_ta[c] = s[2 + 2 * c] & 15;
                if (h.comp_td[c] > 3 || h.comp_ta[c] > 3) bad("Huffman table number", seg);
            }
            if (s[1 + 2 * nc] != 0 || s[2 + 2 * nc] != 63 || s[3 + 2 * nc] != 0)
                return unsupported(h, MVP_JPEG_PROCESS);
            // libjpeg's colour space rule (default_decompress_parms): JFIF says YCbCr; an Adobe
            // marker or the component ids 'R' 'G' 'B' may say otherwise
            if (nc == 3 && (h.adobe || (!h.jfif && h.comp_id[0] == 'R' && h.comp_id[1] == 'G' && h.comp_id[2] == 'B')))
                return unsupported(h, MVP_JPEG_COLOUR);
            for (int c = 0; c < nc; c++) {
                if (!h.qt_seen[h.comp_tq[c]]) bad("quantisation table not defined", seg);
                for (int cls = 0; cls < 2; cls++) {
                    const int slot = cls ? h.comp_ta[c] : h.comp_td[c];
                    if (!h.huff[cls][slot].defined) {
                        if (slot > 1) bad("Huffman table not defined", seg);
                        h.huff[cls][slot] = standard_table(cls, slot);
                    }
                }
            }
            h.info.blocks = geometry(h.info.width, h.info.height, nc, h.info.h_samp, h.info.v_samp).blocks;
            h.scan = p;
            return;
        }
        // APPn, COM and anything else with a length: skipped
    }
}

// MSB-first bit reader over entropy-coded data: removes 0xFF00 stuffing and fill bytes, stops
// at a marker (or the end) and feeds zero bits from there on, counting them: a decode that
// consumed any of them ran out of data.
struct Bits {
    const uint8_t* p;
    const uint8_t* end;
    uint64_t buf = 0;
    int cnt = 0;      // valid bits in buf (its low cnt bits)
    int pad = 0;      // zero bits fed since the data ran out (the newest bits of buf)
    bool hit = false; // at a marker (p points at its 0xFF) or at the end

    void refill() {
        while (cnt <= 56) {
            unsigned b = 0;
            if (!hit && p < end) {
                b = *p++;
                if (b == 0xFF) {
                    while (p < end && *p == 0xFF) p++;
                    if (p >= end) {
                        hit = true;
                        b = 0;
                    } else if (*p == 0) {
                        p++;
                    } else {
                        hit = true;
                        p--;
                        b = 0;
                    }
                }
            } else {
                hit = true;
            }
            if (hit) pad += 8;
            buf = buf << 8 | b;
            cnt += 8;
        }
    }
    unsigned peek(int n) const { return (unsigned)(buf >> (cnt - n)) & ((1u << n) - 1); }
    void skip(int n) { cnt -= n; }
    bool overrun() const { return cnt < pad; }
    int real() const { return cnt - pad; }
};

inline int decode_symbol(Bits& b, const Huff& t) {
    const unsigned e = t.look[b.peek(LOOK)];
    if (e) {
        b.skip((int)(e >> 8));
        return (int)(e & 255);
    }
    const int v16 = (int)b.peek(16);
    for (int l = LOOK + 1; l <= 16; l++) {
        const int code = v16 >> (16 - l);
        if (code <= t.maxcode[l]) {
            b.skip(l);
            return t.vals[(code + t.valoff[l]) & 255];
        }
    }
    return -1;
}

inline int receive_extend(Bits& b, int s) {
    const int v = (int)b.peek(s);
    b.skip(s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// Decodes the scan.  Emit: offsets (blocks + 1) and entries are written; otherwise only the
// range condition is checked.  Returns the number of entries; sets info.status = RANGE (and
// stops) when a dequantised coefficient leaves int16.
template <bool Emit>
int64_t decode_scan(const uint8_t* d, size_t n, Header& h, uint32_t* off, uint32_t* coef, int64_t coef_cap) {
    const Geometry g = geometry(h.info.width, h.info.height, h.info.components, h.info.h_samp, h.info.v_samp);
    Bits b{d + h.scan, d + n};
    int pred[3] = {0, 0, 0};
    int64_t k_out = 0;
    int blk = 0;
    const int n_mcu = g.mcu_w * g.mcu_h;
    int until_restart = h.restart ? h.restart : -1, rst = 0;
    for (int m = 0; m < n_mcu; m++) {
        if (until_restart == 0) {
            b.refill();
            if (b.overrun() || !b.hit || b.real() >= 8) bad("restart marker expected", (size_t)(b.p - d));
            if (b.p + 1 >= b.end || b.p[1] != 0xD0 + (rst & 7)) bad("wrong restart marker", (size_t)(b.p - d));
            b = Bits{b.p + 2, d + n};
            rst++;
            pred[0] = pred[1] = pred[2] = 0;
            until_restart = h.restart;
        }
        if (until_restart > 0) until_restart--;
        for (int j = 0; j < g.per_mcu; j++, blk++) {
            const int c = j < g.hs * g.vs ? 0 : j - g.hs * g.vs + 1;
            const Huff& dc = h.huff[0][h.comp_td[c]];
            const Huff& ac = h.huff[1][h.comp_ta[c]];
            const uint16_t* q = h.qt[h.comp_tq[c]];
            if (Emit) off[blk] = (uint32_t)k_out;
            b.refill();
            int s = decode_symbol(b, dc);
            if (s < 0 || s > 15) bad("bad DC code", (size_t)(b.p - d));
            if (s) pred[c] += receive_extend(b, s);
            const int dcv = pred[c];
            if (dcv) {
                const int64_t dq = (int64_t)dcv * q[0];
                if (dcv < -32768 || dcv > 32767 || dq < -32768 || dq > 32767) {
                    if (b.overrun()) bad("scan data ends inside a block", n);
                    h.info.status = MVP_JPEG_RANGE;
                    return 0;
                }
                if (Emit) {
                    if (k_out >= coef_cap) bad("more coefficients than the scan's bytes can hold", (size_t)(b.p - d));
                    coef[k_out] = coef_entry(0, dcv);
                }
                k_out++;
            }
            for (int k = 1; k < 64;) {
                b.refill();
                const int rs = decode_symbol(b, ac);
                if (rs < 0) bad("bad AC code", (size_t)(b.p - d));
                const int r = rs >> 4;
                s = rs & 15;
                if (!s) {
                    if (r != 15) break;
                    k += 16;
                    continue;
                }
                k += r;
                if (k > 63) bad("coefficient index past the block", (size_t)(b.p - d));
                const int v = receive_extend(b, s);
                const int pos = kNatural[k++];
                const int dq = v * q[pos];
                if (dq < -32768 || dq > 32767) {
                    if (b.overrun()) bad("scan data ends inside a block", n);
                    h.info.status = MVP_JPEG_RANGE;
                    return 0;
                }
                if (Emit) {
                    if (k_out >= coef_cap) bad("more coefficients than the scan's bytes can hold", (size_t)(b.p - d));
                    coef[k_out] = coef_entry(pos, v);
                }
                k_out++;
            }
            if (b.overrun()) bad("scan data ends inside a block", n);
        }
    }
    if (Emit) off[blk] = (uint32_t)k_out;
    // what follows the scan must be EOI (bytes after it are ignored); tables or another scan
    // mean a multi-scan file
    const uint8_t* p = b.p;
    const uint8_t* end = d + n;
    for (;;) {
        while (p < end && *p != 0xFF) p++;
        while (p < end && *p == 0xFF) p++;
        if (p >= end) bad("no EOI marker", n);
        if (*p != 0) break;
        p++;
    }
    if (*p == 0xDA || *p == 0xC4 || *p == 0xDB || *p == 0xDD) {
        h.info.status = MVP_JPEG_SCANS;
        return 0;
    }
    if (*p != 0xD9) bad("EOI marker expected", (size_t)(p - d));
    return k_out;
}

}  // namespace
}  // namespace jpeg

extern "C" int mvp_jpeg_info(const uint8_t* data, size_t bytes, int check_range, mvp_jpeg_frame_info* info) {
    MVP_ABI_BEGIN
    MVP_REQUIRE(data && info, "mvp_jpeg_info: NULL pointer");
    jpeg::Header h;
    jpeg::parse_header(data, bytes, h);
    if (check_range && h.info.status == MVP_JPEG_OK) jpeg::decode_scan<false>(data, bytes, h, nullptr, nullptr, 0);
    *info = h.info;
    MVP_ABI_END
}

namespace jpeg {
namespace {

// Entries a frame's scan can hold: every entry takes two bits of it but for one a block (whose
// DC code may be a single bit), and 64 fill a block; + 64 for a block that runs out of data
// (found out at its end).
int64_t entry_bound(int blocks, size_t bytes) {
    const int64_t by_bits = 4 * (int64_t)bytes + blocks, by_blocks = 64 * (int64_t)blocks;
    return (by_bits < by_blocks ? by_bits : by_blocks) + 64;
}

// mvp_jpeg_parse's body.  fits: when given, a coefficient buffer too small for the frame's bound
// clears it and nothing is parsed; without it that is an argument error.
void parse_frame(const uint8_t* data, size_t bytes, mvp_jpeg_frame_info* info, uint16_t* qt_out, uint32_t* off_out,
                 int64_t off_cap, uint32_t* coef_out, int64_t coef_cap, int64_t* n_coef, bool* fits) {
    Header h;
    *n_coef = 0;
    parse_header(data, bytes, h);
    if (h.info.status == MVP_JPEG_OK) {
        MVP_REQUIRE(off_cap > h.info.blocks, "mvp_jpeg_parse: %lld offsets for %d blocks (+ 1)", (long long)off_cap,
                    h.info.blocks);
        const int64_t need = entry_bound(h.info.blocks, bytes);
        if (fits && coef_cap < need) {
            *fits = false;
            return;
        }
        MVP_REQUIRE(coef_cap >= need, "mvp_jpeg_parse: %lld coefficient entries, this frame may take %lld",
                    (long long)coef_cap, (long long)need);
        const int64_t nc = decode_scan<true>(data, bytes, h, off_out, coef_out, coef_cap);
        if (h.info.status == MVP_JPEG_OK) {
            *n_coef = nc;
            std::memset(qt_out, 0, 3 * 64 * sizeof(uint16_t));
            for (int c = 0; c < h.info.components; c++)
                std::memcpy(qt_out + 64 * c, h.qt[h.comp_tq[c]], 64 * sizeof(uint16_t));
        }
    }
    *info = h.info;
}

}  // namespace
}  // namespace jpeg

extern "C" int mvp_jpeg_parse(const uint8_t* data, size_t bytes, mvp_jpeg_frame_info* info, uint16_t* qt_out,
                              uint32_t* off_out, int64_t off_cap, uint32_t* coef_out, int64_t coef_cap,
                              int64_t* n_coef) {
    MVP_ABI_BEGIN
    MVP_REQUIRE(data && info && qt_out && off_out && coef_out && n_coef, "mvp_jpeg_parse: NULL pointer");
    jpeg::parse_frame(data, bytes, info, qt_out, off_out, off_cap, coef_out, coef_cap, n_coef, nullptr);
    MVP_ABI_END
}

extern "C" int mvp_jpeg_scratch(int width, int height, int* blocks, int64_t* plane_bytes) {
    MVP_ABI_BEGIN
    MVP_REQUIRE(blocks && plane_bytes, "mvp_jpeg_scratch: NULL pointer");
    MVP_REQUIRE(width > 0 && height > 0 && width <= 65535 && height <= 65535, "mvp_jpeg_scratch: frame %dx%d", width,
                height);
    jpeg::worst_case(width, height, blocks, plane_bytes);
    MVP_ABI_END
}

extern "C" int mvp_jpeg_parse_many(int n, const uint8_t* const* data, const size_t* bytes, mvp_jpeg_frame_info* info,
                                   uint16_t* qt_out, uint32_t* off_out, int64_t off_stride, uint32_t* coef_out,
                                   int64_t coef_cap, int64_t* n_coef, int* n_done) {
    MVP_ABI_BEGIN
    MVP_REQUIRE(n >= 0 && n_done && (n == 0 || (data && bytes && info && qt_out && off_out && coef_out && n_coef)),
                "mvp_jpeg_parse_many: NULL pointer");
    MVP_REQUIRE(off_stride > 0, "mvp_jpeg_parse_many: offset stride %lld", (long long)off_stride);
    int64_t used = 0;
    *n_done = 0;
    for (int k = 0; k < n; k++) {
        MVP_REQUIRE(data[k], "mvp_jpeg_parse_many: NULL frame %d", k);
        bool fits = true;
        jpeg::parse_frame(data[k], bytes[k], &info[k], qt_out + (size_t)k * 192, off_out + k * off_stride, off_stride,
                          coef_out + used, coef_cap - used, &n_coef[k], &fits);
        if (!fits) break;  // the caller goes on from frame k with more room
        used += n_coef[k];
        *n_done = k + 1;
    }
    MVP_ABI_END
}
