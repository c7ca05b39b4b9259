// gol-mi355x: rule strings (see rule.hpp).
#include "gol/rule.hpp"

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

Rule Rule::from_code(u32 code) {
    if (code & 0xC000u) bad(strprintf("(code 0x%x)", code), "unknown neighbourhood");
    return from_masks(code & 0x0FFFu, (code >> 16) & 0xFFFFu, (Nbhd)((code >> 12) & 3u));
}

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
        for (; i < low.size() && std::isdigit((unsigned char)low[i]); ++i) {
            const int d = low[i] - '0';
            if (d > 8) bad(s, "digit 9: neighbour counts run from 0 to 8");
            if (mask[which] & (1u << d)) bad(s, strprintf("digit %d repeated", d));
            mask[which] |= 1u << d;
        }
    }
    Nbhd nbhd = Nbhd::Moore;  // the suffix, directly after the second list
    if (i < low.size() && (low[i] == 'v' || low[i] == 'h')) nbhd = low[i++] == 'v' ? Nbhd::VonNeumann : Nbhd::Hex;
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
    return r;
}

std::string Rule::str() const {
    std::string out = "B";
    for (int d = 0; d <= 8; ++d)
        if (birth & (1u << d)) out += (char)('0' + d);
    out += "/S";
    for (int d = 0; d <= 8; ++d)
        if (survive & (1u << d)) out += (char)('0' + d);
    return out + nbhd_suffix(nbhd);
}

}  // namespace gol
