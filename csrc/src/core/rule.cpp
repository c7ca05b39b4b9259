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

}  // namespace

Rule Rule::parse(const std::string& s) {
    std::string low;
    for (char c : s) low += (char)std::tolower((unsigned char)c);
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
