// gol-mi355x: host-side tests of the RLE pattern reader and writer (no GPU needed).  Run: build/gol_rle_unit
//
// Covers: round trips of random patterns, counted '$', short rows and rows missing at the end, every
// rejection (with the offending character or offset named), the writer's 70-column lines, S/B rule headers.
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "gol/rle.hpp"

using namespace gol;

static int g_fail = 0, g_pass = 0;
#define CHECK(c)                                                                          \
    do {                                                                                  \
        if (!(c)) {                                                                       \
            if (g_fail < 20) fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++g_fail;                                                                     \
        } else {                                                                          \
            ++g_pass;                                                                     \
        }                                                                                 \
    } while (0)

static RlePattern random_pattern(i64 rows, i64 cols, unsigned seed, double density) {
    std::mt19937_64 rng(seed);
    std::bernoulli_distribution live(density);
    RlePattern p;
    p.rows = rows;
    p.cols = cols;
    p.words.assign((size_t)(rows * p.nw()), 0);
    for (i64 r = 0; r < rows; ++r)
        for (i64 c = 0; c < cols; ++c)
            if (live(rng)) p.set(r, c);
    return p;
}

static bool same(const RlePattern& a, const RlePattern& b) {
    return a.rows == b.rows && a.cols == b.cols && a.rule == b.rule && a.words == b.words;
}

// rows of '.' and 'O' -> pattern
static RlePattern from_rows(const std::vector<std::string>& rows) {
    RlePattern p;
    p.rows = (i64)rows.size();
    p.cols = (i64)rows[0].size();
    p.words.assign((size_t)(p.rows * p.nw()), 0);
    for (i64 r = 0; r < p.rows; ++r)
        for (i64 c = 0; c < p.cols; ++c)
            if (rows[(size_t)r][(size_t)c] == 'O') p.set(r, c);
    return p;
}

// the text must be refused, with an error that holds `needle` (the offending character or its offset)
static void check_rejected(const std::string& text, const std::string& needle) {
    bool threw = false, named = false;
    std::string what;
    try {
        parse_rle(text);
    } catch (const Error& e) {
        threw = true;
        what = e.what();
        named = what.find(needle) != std::string::npos;
    }
    if (!threw) fprintf(stderr, "accepted: %s\n", text.c_str());
    if (threw && !named) fprintf(stderr, "error '%s' does not name '%s'\n", what.c_str(), needle.c_str());
    CHECK(threw);
    CHECK(named);
}

static void test_round_trips() {
    const i64 sizes[][2] = {{1, 1}, {1, 65}, {64, 64}, {65, 3}, {70, 200}};
    unsigned seed = 1;
    for (const auto& s : sizes)
        for (double density : {0.0, 0.05, 0.5, 0.95, 1.0})
            for (const char* rule : {"", "B3/S23", "B36/S23"}) {
                RlePattern p = random_pattern(s[0], s[1], seed++, density);
                p.rule = rule;
                const std::string text = write_rle(p);
                CHECK(same(parse_rle(text), p));
                CHECK(write_rle(parse_rle(text)) == text);
                CHECK(text.size() >= 2 && text[text.size() - 2] == '!');
            }
}

static void test_reader_forms() {
    const RlePattern glider = from_rows({".O.", "..O", "OOO"});
    CHECK(same(parse_rle("x = 3, y = 3\nbob$2bo$3o!"), glider));
    CHECK(same(parse_rle("#N Glider\n#C a comment, x = 9\n\nx=3,y=3\nbob$2bo$3o!\n"), glider));
    CHECK(same(parse_rle("  x  =  3 ,y= 3\r\nb o b $\n2b\to$\n\n3o ! this text is ignored: 5z$"), glider));
    CHECK(same(parse_rle("x = 3, y = 3\nbo$2bo$3o!"), glider));  // a short row is dead-padded
    RlePattern g2 = glider;
    g2.rule = "B3/S23";
    CHECK(same(parse_rle("x = 3, y = 3, rule = B3/S23\nbob$2bo$3o!"), g2));
    CHECK(same(parse_rle("X = 3, Y = 3, RULE = b3/s23\nbob$2bo$3o!"), g2));
    // counted '$' skips rows; rows missing at the end are dead
    CHECK(same(parse_rle("x = 3, y = 6\n3o3$obo!"), from_rows({"OOO", "...", "...", "O.O", "...", "..."})));
    CHECK(same(parse_rle("x = 3, y = 4\n2$o!"), from_rows({"...", "...", "O..", "..."})));
    CHECK(same(parse_rle("x = 2, y = 2\n!"), from_rows({"..", ".."})));
    CHECK(same(parse_rle("x = 2, y = 2\n2o$2o$!"), from_rows({"OO", "OO"})));  // a '$' after the last row
    // a run may be longer than a word and start anywhere
    const RlePattern wide = parse_rle("x = 200, y = 1\n63b70o67b!");
    for (i64 c = 0; c < 200; ++c) CHECK(wide.cell(0, c) == (c >= 63 && c < 133));
    // the writer: no trailing dead cells, blank rows as a counted '$', no trailing dead rows
    CHECK(write_rle(from_rows({"OOO", "...", "...", "O..", "..."})) == "x = 3, y = 5\n3o3$o!\n");
    CHECK(write_rle(from_rows({"...", ".O."})) == "x = 3, y = 2\n$bo!\n");
    CHECK(write_rle(g2) == "x = 3, y = 3, rule = B3/S23\nbo$2bo$3o!\n");
}

static void test_rejections() {
    // a missing header
    check_rejected("", "offset 0");
    check_rejected("#C only a comment\n", "missing header");
    check_rejected("bob$2bo$3o!", "'b'");
    check_rejected("#C c\nbob$2bo$3o!", "offset 5");
    check_rejected("x = 3\nbob!", "header");
    check_rejected("x = 3, z = 3\nbob!", "'z'");
    check_rejected("x = 3, y = 3, rules = B3/S23\nbob!", "'s'");
    check_rejected("x = 0, y = 3\n!", "x = 0");
    // a run that passes x or y
    check_rejected("x = 3, y = 3\n4o!", "passes x = 3");
    check_rejected("x = 3, y = 3\n2o2b!", "offset 16");
    check_rejected("x = 3, y = 3\no$o$o$o!", "passes y = 3");
    check_rejected("x = 3, y = 3\no4$!", "passes y = 3");
    check_rejected("x = 3, y = 3\n3$b!", "offset 15");
    // an unknown tag
    check_rejected("x = 3, y = 3\nbob$2bx$3o!", "'x'");
    check_rejected("x = 3, y = 3\nbob$2bx$3o!", "offset 19");
    check_rejected("x = 3, y = 3\nbOb!", "'O'");
    check_rejected("x = 3, y = 3\nbo.!", "'.'");
    // a count overflow
    check_rejected("x = 3, y = 3\n99999999999999999999999999o!", "overflow");
    check_rejected("x = 3, y = 3\n18446744073709551617o!", "overflow");
    check_rejected("x = 99999999999999999999, y = 3\no!", "overflow");
    check_rejected("x = 1000000000, y = 1000000000\no!", "beyond");
    // a missing '!'
    check_rejected("x = 3, y = 3\nbob$2bo$3o", "missing '!'");
    check_rejected("x = 3, y = 3\nbob$2bo$3o\n", "offset 24");
    // a rule Rule::parse refuses
    check_rejected("x = 3, y = 3, rule = B39/S23\no!", "B39/S23");
    check_rejected("x = 3, y = 3, rule = 23/0\no!", "23/0");  // S23/B0
    check_rejected("x = 3, y = 3, rule = LifeHistory\no!", "LifeHistory");
}

static void test_line_limit() {
    for (unsigned seed = 0; seed < 4; ++seed) {
        const std::string text = write_rle(random_pattern(70, 200, 100 + seed, 0.5));
        std::istringstream in(text);
        std::string line;
        size_t lines = 0, longest = 0;
        while (std::getline(in, line)) {
            ++lines;
            if (lines > 1) longest = std::max(longest, line.size());  // (the header is one line whatever its length)
            CHECK(lines == 1 || line.size() <= 70);
        }
        CHECK(lines > 10 && longest > 60);  // the lines are filled, not merely short
    }
    // one long run: the tokens are never split across lines
    RlePattern p = random_pattern(3, 4000, 7, 0.5);
    const std::string text = write_rle(p);
    CHECK(same(parse_rle(text), p));
}

static void test_rules() {
    auto rule_of = [](const std::string& r) { return parse_rle("x = 1, y = 1, rule = " + r + "\no!").rule; };
    CHECK(rule_of("B3/S23") == "B3/S23");
    CHECK(rule_of("23/3") == "B3/S23");  // the S/B form Golly writes
    CHECK(rule_of("23/36") == "B36/S23");
    CHECK(rule_of("/2") == "B2/S");
    CHECK(rule_of("012345678/3") == "B3/S012345678");
    CHECK(rule_of("s23/b36") == "B36/S23");
    CHECK(rule_of("highlife") == "B36/S23");
    CHECK(rule_of("  B3678/S34678  ") == "B3678/S34678");
    CHECK(parse_rle("x = 1, y = 1\no!").rule.empty());
}

static void test_files() {
    const std::string path = "gol_rle_unit_tmp.rle";
    RlePattern p = random_pattern(33, 130, 5, 0.3);
    p.rule = "B36/S23";
    write_rle_file(path, p);
    CHECK(same(read_rle_file(path), p));
    remove(path.c_str());
    bool threw = false;
    try {
        read_rle_file("no/such/file.rle");
    } catch (const Error& e) {
        threw = std::string(e.what()).find("no/such/file.rle") != std::string::npos;
    }
    CHECK(threw);
}

int main() {
    test_round_trips();
    test_reader_forms();
    test_rejections();
    test_line_limit();
    test_rules();
    test_files();
    printf("gol_rle_unit: %d passed, %d failed\n", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
