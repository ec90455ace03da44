// Stand-alone driver of csrc/host_mont.h for tests/test_host_field.py: reads one case per line from stdin, writes one answer per line.
//     <field: r | q> <op> <hex operand> [<hex operand>]
// Operands are 256-bit integers as 64 hex digits.  Values enter through from_words and leave through to_words unless the op says otherwise.
#include <stdio.h>
#include <string.h>

#include "host_mont.h"

using namespace gl355;

static bool parse(const char* s, uint64_t w[4]) {
    if (strlen(s) != 64) return false;
    for (int i = 0; i < 4; i++) {
        w[3 - i] = 0;
        for (int k = 0; k < 16; k++) {
            const char c = s[16 * i + k];
            const int d = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1;
            if (d < 0) return false;
            w[3 - i] = (w[3 - i] << 4) | (uint64_t)d;
        }
    }
    return true;
}
static void put(const uint64_t w[4]) { printf("%016llx%016llx%016llx%016llx\n", (unsigned long long)w[3], (unsigned long long)w[2], (unsigned long long)w[1], (unsigned long long)w[0]); }

template <class F>
static bool run(const char* op, const uint64_t a[4], const uint64_t b[4], bool has_b) {
    uint64_t o[4];
    const F x = F::from_words(a), y = has_b ? F::from_words(b) : F::zero();
    if (!strcmp(op, "mul") && has_b) (x * y).to_words(o);
    else if (!strcmp(op, "add") && has_b) (x + y).to_words(o);
    else if (!strcmp(op, "sub") && has_b) (x - y).to_words(o);
    else if (!strcmp(op, "lt") && has_b) { printf("%d\n", x.less_than(y) ? 1 : 0); return true; }
    else if (!strcmp(op, "eq") && has_b) { printf("%d\n", (x == y ? 1 : 0) | (x != y ? 2 : 0)); return true; }
    else if (!strcmp(op, "pow") && has_b) x.pow(b).to_words(o);                  // b: the raw exponent
    else if (!strcmp(op, "neg")) x.neg().to_words(o);
    else if (!strcmp(op, "inv")) x.inv().to_words(o);
    else if (!strcmp(op, "zero")) { printf("%d\n", x.is_zero() ? 1 : 0); return true; }
    else if (!strcmp(op, "words")) x.to_words(o);                                // to_words(from_words(a))
    else if (!strcmp(op, "mont")) memcpy(o, F::from_mont_words(a).l, 32);        // the limbs themselves: a mod m
    else return false;
    put(o);
    return true;
}

int main() {
    char line[256], f[8], op[16], sa[80], sb[80];
    while (fgets(line, sizeof line, stdin)) {
        const int n = sscanf(line, "%7s %15s %79s %79s", f, op, sa, sb);
        uint64_t a[4], b[4] = {0, 0, 0, 0};
        if (n == 3 && !strcmp(f, "r") && !strcmp(op, "root")) {                  // Fr::root_of_unity(decimal k)
            uint64_t o[4];
            unsigned k = 0;
            if (sscanf(sa, "%u", &k) != 1 || k > BN254C_FR_S) { fprintf(stderr, "bad case: %s", line); return 2; }
            Fr::root_of_unity(k).to_words(o);
            put(o);
            continue;
        }
        bool ok = n >= 3 && parse(sa, a) && (n < 4 || parse(sb, b));
        if (ok && !strcmp(f, "r")) ok = run<Fr>(op, a, b, n == 4);
        else if (ok && !strcmp(f, "q")) ok = run<Fq>(op, a, b, n == 4);
        else ok = false;
        if (!ok) { fprintf(stderr, "bad case: %s", line); return 2; }
    }
    return 0;
}
