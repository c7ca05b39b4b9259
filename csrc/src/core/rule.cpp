// gol-mi355x: rule strings (see rule.hpp).
#include "gol/rule.hpp"

#include <algorithm>
#include <cctype>

namespace gol {

namespace {

const char* kB0Text =
    "B0 rules are out of scope: the dead background would come alive, and the engine's zeroed slack rows, trash "
    "lanes and masked tail bits assume dead stays dead";

[[noreturn]] void bad(const std::string& s, const std::string& why) {
    throw Error("invalid rule '" + s + "': " + why);
}

}  // namespace

const char* nbhd_name(Nbhd n) {
    return n == Nbhd::VonNeumann ? "von Neumann" : (n == Nbhd::Hex ? "hexagonal" : "Moore");
}

Rule Rule::from_masks(unsigned birth, unsigned survive) { return from_masks(birth, survive, Nbhd::Moore); }

Rule Rule::from_masks(unsigned birth, unsigned survive, Nbhd nbhd) {
    if ((unsigned)nbhd > (unsigned)Nbhd::Hex)
        bad(strprintf("(birth 0x%x, survive 0x%x)", birth, survive), strprintf("unknown neighbourhood %u", (unsigned)nbhd));
    const std::string name = nbhd == Nbhd::Moore
                                 ? strprintf("(birth 0x%x, survive 0x%x)", birth, survive)
                                 : strprintf("(birth 0x%x, survive 0x%x, %s)", birth, survive, nbhd_name(nbhd));
    const unsigned top = (2u << nbhd_max_count(nbhd)) - 1u;
    if (birth > top || survive > top) bad(name, strprintf("neighbour counts run from 0 to %d", nbhd_max_count(nbhd)));
    if (birth & 1u) bad(name, kB0Text);
    Rule r;
    r.birth = (u16)birth;
    r.survive = (u16)survive;
    r.nbhd = nbhd;
    return r;
}

Rule Rule::from_masks(unsigned birth, unsigned survive, Nbhd nbhd, unsigned states) {
    Rule r = from_masks(birth, survive, nbhd);
    const std::string name = strprintf("(birth 0x%x, survive 0x%x, %u states)", birth, survive, states);
    if (states < 2 || states > (unsigned)kMaxStates)
        bad(name, strprintf("a rule has 2 states or, as a Generations rule, 3 to %d", kMaxStates));
    if (states > 2 && nbhd != Nbhd::Moore)
        bad(name, strprintf("Generations rules count the Moore neighbourhood only, not the %s one", nbhd_name(nbhd)));
    r.states = (u16)states;
    return r;
}

Rule Rule::from_code(u32 code) {
    if (code & 0xC000u) bad(strprintf("(code 0x%x)", code), "unknown neighbourhood");
    if (code & 0x80000000u) bad(strprintf("(code 0x%x)", code), "unknown rule family");
    return from_masks(code & 0x0FFFu, (code >> 16) & 0x0FFFu, (Nbhd)((code >> 12) & 3u), ((code >> 28) & 7u) + 2u);
}

namespace {

// The digits of one list from low[i] on into `mask` (i moves past them).
void read_digits(const std::string& s, const std::string& low, size_t& i, unsigned& mask) {
    for (; i < low.size() && std::isdigit((unsigned char)low[i]); ++i) {
        const int d = low[i] - '0';
        if (d > 8) bad(s, "digit 9: neighbour counts run from 0 to 8");
        if (mask & (1u << d)) bad(s, strprintf("digit %d repeated", d));
        mask |= 1u << d;
    }
}

// The state count of a Generations rule from low[i] on (i moves past it): 2 .. 9, no leading zeros, not empty.
unsigned read_states(const std::string& s, const std::string& low, size_t& i) {
    const size_t at = i;
    while (i < low.size() && std::isdigit((unsigned char)low[i])) ++i;
    const std::string n = low.substr(at, i - at);
    if (n.empty()) bad(s, "the state count after /C is missing");
    if (n.size() > 1 && n[0] == '0') bad(s, "the state count '" + n + "' has a leading zero");
    if (n.size() > 1 || n[0] < '2')
        bad(s, strprintf("%s states: a Generations rule has 3 to %d (C2 is the two-state rule)", n.c_str(), Rule::kMaxStates));
    return (unsigned)(n[0] - '0');
}

// A number of an LtL field: digits only, not empty, no leading zero, at most four digits.
unsigned ltl_number(const std::string& s, const std::string& text, const char* what) {
    if (text.empty()) bad(s, std::string("the number of ") + what + " is missing");
    for (char c : text)
        if (!std::isdigit((unsigned char)c)) bad(s, std::string("'") + text + "' in " + what + " is not a number");
    if (text.size() > 1 && text[0] == '0') bad(s, std::string("'") + text + "' in " + what + " has a leading zero");
    if (text.size() > 4) bad(s, std::string("'") + text + "' in " + what + " is out of range");
    return (unsigned)std::stoul(text);
}

// The checks of an LtL rule's numbers, shared by the parser and from_ltl; `s` names the rule in the error.
Rule checked_ltl(const std::string& s, unsigned r, unsigned c, unsigned m, unsigned smin, unsigned smax, unsigned bmin,
                 unsigned bmax) {
    if (r < 1 || r > (unsigned)Rule::kMaxRange)
        bad(s, strprintf("range R%u: Larger than Life rules run with R1 to R%d (a count of up to (2*%d+1)^2 = 225 fits 8 bit planes)",
                         r, Rule::kMaxRange, Rule::kMaxRange));
    if (c >= 3) bad(s, strprintf("C%u: Larger than Life rules with history states (C >= 3) are not built; C0 or C2 (two states)", c));
    if (c == 1) bad(s, "C1: the state count of a Larger than Life rule is C0 or C2 (two states)");
    if (m > 1) bad(s, strprintf("M%u: the middle flag is M0 (the cell itself is not counted) or M1", m));
    const unsigned box = (2 * r + 1) * (2 * r + 1);
    if (smin > smax || smax > box)
        bad(s, strprintf("S%u..%u: an interval needs min <= max <= (2*%u+1)^2 = %u", smin, smax, r, box));
    if (bmin > bmax || bmax > box)
        bad(s, strprintf("B%u..%u: an interval needs min <= max <= (2*%u+1)^2 = %u", bmin, bmax, r, box));
    if (bmin == 0) bad(s, kB0Text);
    Rule out;
    out.birth = 0;
    out.survive = 0;
    out.range = (u16)r;
    out.middle = (u16)m;
    out.smin = (u16)smin;
    out.smax = (u16)smax;
    out.bmin = (u16)bmin;
    out.bmax = (u16)bmax;
    return out;
}

// "r<r>,c<c>,m<m>,s<min>..<max>,b<min>..<max>[,n<n>]" (lower case already; `s` is the string as given).
Rule parse_ltl(const std::string& s, const std::string& low) {
    if (low.find(' ') != std::string::npos || low.find('\t') != std::string::npos) bad(s, "spaces in a Larger than Life rule");
    if (low.back() == ',') bad(s, "a trailing comma");
    std::string order;
    unsigned num[5] = {0, 0, 0, 0, 0}, top[2] = {0, 0};  // r, c, m, smin, bmin; smax, bmax
    for (size_t at = 0; at <= low.size();) {
        size_t end = low.find(',', at);
        if (end == std::string::npos) end = low.size();
        const std::string f = low.substr(at, end - at);
        at = end + 1;
        if (f.empty()) bad(s, "an empty field");
        const char l = f[0];
        const std::string rest = f.substr(1);
        if (std::string("rcmsbn").find(l) == std::string::npos)
            bad(s, std::string("unknown field '") + f + "' (the fields are R, C, M, S, B and N)");
        if (order.find(l) != std::string::npos) bad(s, strprintf("field %c twice", (char)std::toupper((unsigned char)l)));
        order += l;
        if (l == 'n') {
            if (rest == "n") bad(s, "NN, the von Neumann neighbourhood of range R, is not built; NM (the box) only");
            if (rest == "c") bad(s, "NC, the circular neighbourhood of range R, is not built; NM (the box) only");
            if (rest != "m") bad(s, "neighbourhood '" + f + "': NM (the box) only");
        } else if (l == 's' || l == 'b') {
            const size_t dots = rest.find("..");
            const char* what = l == 's' ? "S<min>..<max>" : "B<min>..<max>";
            if (dots == std::string::npos) bad(s, std::string("field '") + f + "' is not " + what);
            num[l == 's' ? 3 : 4] = ltl_number(s, rest.substr(0, dots), what);
            top[l == 's' ? 0 : 1] = ltl_number(s, rest.substr(dots + 2), what);
        } else {
            num[l == 'r' ? 0 : (l == 'c' ? 1 : 2)] = ltl_number(s, rest, l == 'r' ? "R<r>" : (l == 'c' ? "C<c>" : "M<m>"));
        }
    }
    for (char l : std::string("rcmsb"))
        if (order.find(l) == std::string::npos) bad(s, strprintf("field %c is missing", (char)std::toupper((unsigned char)l)));
    if (order != "rcmsb" && order != "rcmsbn") bad(s, "the fields come in the order R,C,M,S,B[,N]");
    return checked_ltl(s, num[0], num[1], num[2], num[3], top[0], num[4], top[1]);
}

}  // namespace

Rule Rule::from_ltl(unsigned range, unsigned middle, unsigned smin, unsigned smax, unsigned bmin, unsigned bmax) {
    return checked_ltl(strprintf("(R%u, M%u, S%u..%u, B%u..%u)", range, middle, smin, smax, bmin, bmax), range, 0, middle, smin,
                       smax, bmin, bmax);
}

Rule::LtlThresholds Rule::ltl_thresholds() const {
    const unsigned top = (unsigned)box(), up = 1u - (middle ? 1u : 0u);
    LtlThresholds t;
    t.blo = bmin;
    t.bhi = (u16)std::min<unsigned>(bmax, top);
    t.slo = (u16)(smin + up);
    t.shi = (u16)std::min<unsigned>(smax + up, top);
    if (t.blo > top) t.blo = 1, t.bhi = 0;
    if (t.slo > top) t.slo = 1, t.shi = 0;  // (M0 with smin = (2R+1)^2: no live cell has that many neighbours)
    return t;
}

Rule Rule::parse(const std::string& s) {
    std::string low;
    for (char c : s) low += (char)std::tolower((unsigned char)c);
    if (low == "bosco") low = "r5,c0,m1,s34..58,b34..45,nm";
    // A Larger than Life rule begins with its R field (nothing else begins with r but the alias replicator)
    if (low.size() >= 2 && low[0] == 'r' && low != "replicator") return parse_ltl(s, low);
    static const struct {
        const char* name;
        const char* rule;
    } aliases[] = {{"conway", "b3/s23"},         {"life", "b3/s23"}, {"highlife", "b36/s23"},
                   {"daynight", "b3678/s34678"}, {"seeds", "b2/s"},  {"replicator", "b1357/s1357"}};
    for (const auto& a : aliases)
        if (low == a.name) low = a.rule;
    unsigned mask[2] = {0, 0};  // birth, survive
    bool seen[2] = {false, false};
    size_t i = 0;
    // The bare Generations form <survive digits>/<birth digits>/<states>: digits and exactly two slashes, nothing else.
    if (!low.empty() && low.find_first_not_of("0123456789/") == std::string::npos &&
        std::count(low.begin(), low.end(), '/') == 2) {
        read_digits(s, low, i, mask[1]);
        ++i;  // (the first slash)
        read_digits(s, low, i, mask[0]);
        ++i;
        const unsigned states = read_states(s, low, i);
        if (mask[0] & 1u) bad(s, kB0Text);
        Rule r;
        r.birth = (u16)mask[0];
        r.survive = (u16)mask[1];
        r.states = (u16)states;
        return r;
    }
    for (int part = 0; part < 2; ++part) {
        if (part == 1) {
            if (i >= low.size() || low[i] != '/') bad(s, "expected B<digits>/S<digits>");
            ++i;
        }
        if (i >= low.size() || (low[i] != 'b' && low[i] != 's'))
            bad(s, part == 0 ? "expected B<digits>/S<digits>" : "missing B or S part");
        const int which = low[i] == 'b' ? 0 : 1;
        if (seen[which]) bad(s, which == 0 ? "two B parts, missing S part" : "two S parts, missing B part");
        seen[which] = true;
        ++i;
        read_digits(s, low, i, mask[which]);
    }
    Nbhd nbhd = Nbhd::Moore;  // the suffix, directly after the second list
    if (i < low.size() && (low[i] == 'v' || low[i] == 'h')) nbhd = low[i++] == 'v' ? Nbhd::VonNeumann : Nbhd::Hex;
    unsigned states = 2;  // the third field of a Generations rule: /C<n>
    if (i + 1 < low.size() && low[i] == '/' && low[i + 1] == 'c') {
        i += 2;
        states = read_states(s, low, i);
        if (nbhd != Nbhd::Moore || (i < low.size() && (low[i] == 'v' || low[i] == 'h')))
            bad(s, "a V or H suffix together with /C: Generations rules count the Moore neighbourhood only");
    }
    if (i != low.size()) bad(s, "trailing text '" + s.substr(i) + "'");
    const int top = nbhd_max_count(nbhd);
    for (int d = top + 1; d <= 8; ++d)
        if ((mask[0] | mask[1]) & (1u << d))
            bad(s, strprintf("digit %d: %s neighbour counts run from 0 to %d", d, nbhd_name(nbhd), top));
    if (mask[0] & 1u) bad(s, kB0Text);
    Rule r;
    r.birth = (u16)mask[0];
    r.survive = (u16)mask[1];
    r.nbhd = nbhd;
    r.states = (u16)states;
    return r;
}

std::string Rule::str() const {
    if (ltl())
        return strprintf("R%u,C0,M%u,S%u..%u,B%u..%u,NM", (unsigned)range, (unsigned)middle, (unsigned)smin, (unsigned)smax,
                         (unsigned)bmin, (unsigned)bmax);
    std::string out = "B";
    for (int d = 0; d <= 8; ++d)
        if (birth & (1u << d)) out += (char)('0' + d);
    out += "/S";
    for (int d = 0; d <= 8; ++d)
        if (survive & (1u << d)) out += (char)('0' + d);
    out += nbhd_suffix(nbhd);
    if (states > 2) out += strprintf("/C%u", (unsigned)states);
    return out;
}

}  // namespace gol
