// gol-mi355x: RLE pattern reader and writer (see rle.hpp).  Host only.
#include "gol/rle.hpp"

#include <cctype>
#include <fstream>
#include <sstream>

#include "gol/rule.hpp"

namespace gol {

namespace {

constexpr i64 kMaxCount = (i64)1 << 40;  // a run count beyond this is an overflow, whatever x and y are

std::string show(char c) {
    return std::isprint((unsigned char)c) ? strprintf("'%c'", c) : strprintf("'\\x%02x'", (unsigned)(unsigned char)c);
}

[[noreturn]] void fail(const std::string& what, size_t off) {
    throw Error(strprintf("RLE: %s at offset %zu", what.c_str(), off));
}

bool blank(char c) { return c == ' ' || c == '\t' || c == '\r' || c == '\n' || c == '\f' || c == '\v'; }

// "x = N, y = M[, rule = R]" in text[i, eol); offsets in the errors are offsets into the whole text.
struct Header {
    i64 x = 0, y = 0;
    std::string rule;
};

Header parse_header(const std::string& t, size_t i, size_t eol) {
    auto skip = [&] {
        while (i < eol && blank(t[i])) ++i;
    };
    auto expect = [&](char c) {
        skip();
        if (i >= eol || std::tolower((unsigned char)t[i]) != c)
            fail(strprintf("header: expected '%c', found %s", c, i < eol ? show(t[i]).c_str() : "the end of the line"), i);
        ++i;
    };
    auto number = [&]() {
        skip();
        if (i >= eol || !std::isdigit((unsigned char)t[i]))
            fail(std::string("header: expected a number, found ") + (i < eol ? show(t[i]) : "the end of the line"), i);
        i64 v = 0;
        for (; i < eol && std::isdigit((unsigned char)t[i]); ++i) {
            v = v * 10 + (t[i] - '0');
            if (v > kMaxCount) fail("header: number overflow", i);
        }
        return v;
    };
    Header h;
    expect('x');
    expect('=');
    h.x = number();
    expect(',');
    expect('y');
    expect('=');
    h.y = number();
    skip();
    if (i < eol) {
        expect(',');
        for (char c : {'r', 'u', 'l', 'e'}) expect(c);
        expect('=');
        skip();
        size_t e = eol;
        while (e > i && blank(t[e - 1])) --e;
        if (e == i) fail("header: empty rule", i);
        h.rule = t.substr(i, e - i);
    }
    return h;
}

// The header's rule in canonical form.  Golly also writes the S/B form, survival digits first and no
// letters (23/3); Rule::parse takes only the lettered forms, so that one is rewritten here.
std::string canonical_rule(const std::string& r) {
    std::string s = r;
    const size_t slash = r.find('/');
    if (slash != std::string::npos) {
        // the neighbourhood suffix (V, H) follows the second list in this form too: 34/2H
        const char last = (char)std::toupper((unsigned char)r.back());
        const size_t end = (last == 'V' || last == 'H') && r.size() - 1 > slash ? r.size() - 1 : r.size();
        bool digits = end > 1;
        for (size_t k = 0; k < end; ++k)
            if (k != slash && !std::isdigit((unsigned char)r[k])) digits = false;
        if (digits) s = "B" + r.substr(slash + 1, end - slash - 1) + "/S" + r.substr(0, slash) + r.substr(end);
    }
    try {
        return Rule::parse(s).str();
    } catch (const Error& e) {
        throw Error("RLE: header rule '" + r + "': " + e.what());
    }
}

}  // namespace

RleTopology split_rule_topology(const std::string& field) {
    RleTopology t;
    const size_t colon = field.find(':');
    if (colon == std::string::npos) {
        t.rule = field;
        return t;
    }
    t.rule = field.substr(0, colon);
    while (!t.rule.empty() && blank(t.rule.back())) t.rule.pop_back();
    const std::string sfx = field.substr(colon);
    auto bad = [&](const std::string& why) -> Error {
        return Error("RLE: header topology suffix '" + sfx + "': " + why);
    };
    size_t i = 1;
    if (i >= sfx.size()) throw bad("expected T<w>[,<h>] or P<w>[,<h>]");
    const char kind = (char)std::toupper((unsigned char)sfx[i++]);
    if (kind == 'K' || kind == 'C' || kind == 'S')
        throw bad(std::string("topology ") + kind + " (Klein bottle, cross-surface, sphere) is not supported; only T (torus) and P (plane)");
    if (kind != 'T' && kind != 'P') throw bad("unknown topology " + show(sfx[1]) + "; expected T (torus) or P (plane)");
    auto dimension = [&](const char* name) {
        if (i >= sfx.size() || !std::isdigit((unsigned char)sfx[i])) throw bad(std::string("expected the board's ") + name);
        i64 v = 0;
        for (; i < sfx.size() && std::isdigit((unsigned char)sfx[i]); ++i) {
            v = v * 10 + (sfx[i] - '0');
            if (v > kMaxCount) throw bad("number overflow");
        }
        if (i < sfx.size() && (sfx[i] == '+' || sfx[i] == '-' || sfx[i] == '*'))
            throw bad("shifted or twisted edges (+n, -n, *) are not supported");
        if (v == 0) throw bad(std::string("an infinite ") + name + " (0) is not supported");
        return v;
    };
    t.topology = std::string(1, kind);
    t.cols = dimension("width");
    t.rows = t.cols;  // one number: a square board
    if (i < sfx.size() && sfx[i] == ',') {
        ++i;
        t.rows = dimension("height");
    }
    if (i < sfx.size()) throw bad("unexpected " + show(sfx[i]) + " after the board's size");
    return t;
}

namespace {

void put_run(std::string& out, size_t& line_len, i64 count, char tag) {
    std::string tok = count > 1 ? strprintf("%lld%c", (long long)count, tag) : std::string(1, tag);
    if (line_len + tok.size() > 70) {
        out += '\n';
        line_len = 0;
    }
    out += tok;
    line_len += tok.size();
}

}  // namespace

RlePattern parse_rle(const std::string& text) {
    const size_t n = text.size();
    size_t i = 0;
    for (;;) {  // comment and blank lines before the header
        while (i < n && blank(text[i])) ++i;
        if (i < n && text[i] == '#') {
            while (i < n && text[i] != '\n') ++i;
            continue;
        }
        break;
    }
    if (i >= n) fail("missing header (x = N, y = M): the text ends", i);
    if (text[i] != 'x' && text[i] != 'X') fail("missing header (x = N, y = M): found " + show(text[i]), i);
    size_t eol = text.find('\n', i);
    if (eol == std::string::npos) eol = n;
    const Header hd = parse_header(text, i, eol);
    if (hd.x < 1 || hd.y < 1) fail(strprintf("header: x = %lld, y = %lld (both must be >= 1)", (long long)hd.x, (long long)hd.y), i);
    if (hd.x > kRleMaxCells / hd.y)
        fail(strprintf("header: a %lld x %lld pattern is beyond the reader's %lld cells", (long long)hd.y, (long long)hd.x,
                       (long long)kRleMaxCells), i);
    RlePattern p;
    p.rows = hd.y;
    p.cols = hd.x;
    if (!hd.rule.empty()) {
        const RleTopology topo = split_rule_topology(hd.rule);
        if (topo.rule.empty()) fail("header: empty rule before the topology suffix", i);
        p.rule = canonical_rule(topo.rule);
        p.topology = topo.topology;
        p.bound_cols = topo.cols;
        p.bound_rows = topo.rows;
    }
    const i64 nw = p.nw();
    p.words.assign((size_t)(p.rows * nw), 0);

    i64 row = 0, col = 0, count = 0;
    bool counted = false;
    for (i = eol; i < n; ++i) {
        const char c = text[i];
        if (blank(c)) continue;
        if (std::isdigit((unsigned char)c)) {
            count = count * 10 + (c - '0');
            counted = true;
            if (count > kMaxCount) fail("run count overflow, digit " + show(c), i);
            continue;
        }
        const i64 k = counted ? count : 1;
        count = 0;
        counted = false;
        if (c == '!') return p;
        if (c == '$') {
            row += k;
            col = 0;
            if (row > p.rows) fail(strprintf("run %lld%c passes y = %lld", (long long)k, c, (long long)p.rows), i);
        } else if (c == 'b' || c == 'o') {
            if (k > 0 && row >= p.rows)
                fail(strprintf("run %lld%c in row %lld passes y = %lld", (long long)k, c, (long long)row, (long long)p.rows), i);
            if (k > p.cols - col)
                fail(strprintf("run %lld%c from column %lld passes x = %lld", (long long)k, c, (long long)col, (long long)p.cols), i);
            if (c == 'o') {
                u64* w = &p.words[(size_t)(row * nw)];
                for (i64 x = col; x < col + k; ++x) w[x >> 6] |= 1ull << (x & 63);
            }
            col += k;
        } else {
            fail("unknown tag " + show(c), i);
        }
    }
    fail("missing '!': the text ends", n);
}

std::string write_rle(const RlePattern& p) {
    if (p.rows < 1 || p.cols < 1 || (i64)p.words.size() != p.rows * p.nw())
        throw Error(strprintf("write_rle: a %lld x %lld pattern with %zu words", (long long)p.rows, (long long)p.cols,
                              p.words.size()));
    std::string out = strprintf("x = %lld, y = %lld", (long long)p.cols, (long long)p.rows);
    if (!p.topology.empty()) {
        if ((p.topology != "T" && p.topology != "P") || p.bound_cols < 1 || p.bound_rows < 1)
            throw Error(strprintf("write_rle: topology '%s' with a %lld x %lld board (T or P, both sizes >= 1)", p.topology.c_str(),
                                  (long long)p.bound_rows, (long long)p.bound_cols));
        out += ", rule = " + (p.rule.empty() ? Rule().str() : p.rule) +
               strprintf(":%s%lld,%lld", p.topology.c_str(), (long long)p.bound_cols, (long long)p.bound_rows);
    } else if (!p.rule.empty())
        out += ", rule = " + p.rule;
    out += '\n';
    size_t line_len = 0;
    const i64 nw = p.nw();
    i64 at = 0;  // the row the text stands in
    for (i64 r = 0; r < p.rows; ++r) {
        const u64* w = &p.words[(size_t)(r * nw)];
        i64 last = -1;  // last live column
        for (i64 c = nw - 1; c >= 0 && last < 0; --c) {
            const u64 v = w[c] & word_mask(c, p.cols);
            if (v) last = 64 * c + 63 - __builtin_clzll(v);
        }
        if (last < 0) continue;
        if (r > at) put_run(out, line_len, r - at, '$');
        at = r;
        for (i64 c = 0; c <= last;) {
            const bool live = (w[c >> 6] >> (c & 63)) & 1ull;
            i64 e = c + 1;
            while (e <= last && (((w[e >> 6] >> (e & 63)) & 1ull) != 0) == live) ++e;
            put_run(out, line_len, e - c, live ? 'o' : 'b');
            c = e;
        }
    }
    put_run(out, line_len, 1, '!');
    out += '\n';
    return out;
}

RlePattern read_rle_file(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw Error("cannot open RLE file " + path);
    std::stringstream ss;
    ss << f.rdbuf();
    try {
        return parse_rle(ss.str());
    } catch (const Error& e) {
        throw Error(path + ": " + e.what());
    }
}

void write_rle_file(const std::string& path, const RlePattern& p) {
    const std::string text = write_rle(p);
    std::ofstream f(path, std::ios::binary | std::ios::trunc);
    if (!f || !(f << text) || !f.flush()) throw Error("cannot write RLE file " + path);
}

}  // namespace gol
