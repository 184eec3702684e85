// main_test_pc.cpp -- the reference's commented-out CLI hook `./pigeon <logN> <option> <K>` (option 4: RS x expander, option 1: RS x RS,
// option 3: the Brakedown baseline, K unused) and `elastic <logN> <logB> <opt>` (Elastic_PC options 1 and 2; option 3: the streaming
// Brakedown baseline, which sets its own buffer size, so <logB> is ignored there as in the reference) and `whir <logN>` (the standalone WHIR
// baseline: test_PC's last branch, which test_PC itself keeps refusing) and `brakingbase <logN> <K>` (the Braking base baseline: test_PC's
// option 5, which test_PC itself keeps refusing; shapes outside 4 <= K <= 512, 128 <= N / K <= 2^20 print an error and return 255) and
// `brakingbase_any <logN> <K>` (the same baseline through include/hobbit_longcodes.h: N / K up to 2^21, which `28 5 128` of PC_tests.sh needs) and
// `real <logN> <K>` (option 4 with the polynomial drawn on the device as base-field values of 8 bytes and committed as a half commitment) and
// `real_rs <logN> <K>` (option 1 the same way, include/hobbit_real_rs.h: same root and Ps as `<logN> 1 <K>`) and
// `elastic_real <logN> <logB> <opt>` (Elastic_PC options 1 and 2 on the base-field form of the default streams, 8 bytes per value: every line
// that carries no time equals the line of `elastic <logN> <logB> <opt>`) and
// `orion <logN>` (the Orion baseline: test_PC's option 2, which test_PC itself keeps refusing; logN even in [14, 28], else an error and 255)
// (src/main.cpp:1176: test_PC(1ULL<<atoi(argv[1]), atoi(argv[2]), atoi(argv[3]))) over the
// device-backed host mirror.  Build: see __graft_entry__.build_host().
#include <cstdio>
#include <cstdlib>
#include <string>
#include "hobbit_host.hpp"
int main(int argc, char **argv) {
    const bool whir = argc == 3 && std::string(argv[1]) == "whir";
    const bool bbase = argc == 4 && std::string(argv[1]) == "brakingbase";
    const bool bbase_any = argc == 4 && std::string(argv[1]) == "brakingbase_any";
    const bool orion = argc == 3 && std::string(argv[1]) == "orion";
    const bool real = argc == 4 && std::string(argv[1]) == "real";
    const bool real_rs = argc == 4 && std::string(argv[1]) == "real_rs";
    if (argc < 4 && !whir && !orion) {
        printf("usage: %s <logN> <4 | 1 | 3> <K>   |   %s elastic <logN> <logB> <opt>   |   %s whir <logN>   |   %s brakingbase <logN> <K>   |   %s brakingbase_any <logN> <K>   |   %s orion <logN>   |   %s real <logN> <K>   |   %s elastic_real <logN> <logB> <1 | 2>   |   %s real_rs <logN> <K>\n",
               argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0], argv[0]);
        return 1;
    }
    init_hash();
    if (real_rs) {                                    // option 1 on a base-field polynomial (include/hobbit_real_rs.h): same root and Ps as `<logN> 1 <K>`
        const int logn = atoi(argv[2]), K = atoi(argv[3]);
        const unsigned long long n = 1ULL << (logn < 1 || logn > 40 ? 0 : logn), m = K > 0 ? n / K : 0;
        if (logn < 1 || logn > 40 || K <= 0 || n % K || (m & (m - 1)) || m < 4 * 128 || m > 128ULL << 19) { printf("Error: real_rs takes N = 2^n and K a power of two with 2^9 <= N / K <= 2^26\n"); return 255; }
        test_PC_real_rs(n, K);
    } else
    if (real) {                                       // option 4 on a base-field polynomial (include/hobbit_real.h): same root and Ps as `<logN> 4 <K>`
        const int logn = atoi(argv[2]), K = atoi(argv[3]);
        if (logn < 1 || logn > 40 || K <= 0 || ((1ULL << logn) / K) % 2048 || (1ULL << logn) / K < 2048 * 4) { printf("Error: real takes N = 2^n and K with N / (2048 K) a multiple of 4\n"); return 255; }
        test_PC_real(1ULL << logn, K);
    } else
    if (orion) {                                      // src/Our_PC.cpp:780-793
        const int logn = atoi(argv[2]);
        if (logn < 14 || logn > 28 || (logn & 1)) { printf("Error: Orion takes N = 2^n with n even and 14 <= n <= 28\n"); return 255; }
        test_orion(1ULL << logn);
    } else
    if (bbase_any) {                                  // src/Our_PC.cpp:827-842, rows to 2^21
        const int logn = atoi(argv[2]);
        if (logn < 1 || logn > 40) { printf("Error: Braking base takes N, K powers of two with 4 <= K <= 512 and 128 <= N / K <= 2^21\n"); return 255; }
        test_brakingbase_any(1ULL << logn, atoi(argv[3]));
    } else
    if (bbase) {                                      // src/Our_PC.cpp:827-842
        const int logn = atoi(argv[2]);
        if (logn < 1 || logn > 40) { printf("Error: Braking base takes N, K powers of two with 4 <= K <= 512 and 128 <= N / K <= 2^20\n"); return 255; }
        test_brakingbase(1ULL << logn, atoi(argv[3]));
    } else
    if (whir) {                                       // src/Our_PC.cpp:843-859
        const int logn = atoi(argv[2]);
        if (logn < 9 || logn > 26) { printf("Error: the standalone WHIR baseline takes 9 <= logN <= 26\n"); return 255; }
        test_whir(1ULL << logn);
    } else
    if (std::string(argv[1]) == "elastic_real") {     // include/hobbit_elastic_real.h
        const int opt = argc > 4 ? atoi(argv[4]) : 1;
        if (opt != 1 && opt != 2) { printf("Error: elastic_real takes options 1 and 2\n"); return 255; }
        BUFFER_SPACE = 1ULL << atoi(argv[3]);
        test_Elastic_PC_real(1ULL << atoi(argv[2]), opt);
    } else
    if (std::string(argv[1]) == "elastic") {          // src/main.cpp:1177-1178: BUFFER_SPACE = 1<<argv[2]; test_Elastic_PC(1<<argv[1], argv[3])
        BUFFER_SPACE = 1ULL << atoi(argv[3]);
        test_Elastic_PC(1ULL << atoi(argv[2]), argc > 4 ? atoi(argv[4]) : 1);
    } else
        test_PC(1ULL << atoi(argv[1]), atoi(argv[2]), atoi(argv[3]));
    hobbit_host_shutdown();
    return 0;
}
