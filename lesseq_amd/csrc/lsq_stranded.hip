// The stranded forms of the read-file tools' count kernels: a read counts for the genes or events of its transcript
// strand alone.  The kernels are the templates of the tools' device headers, instantiated here and nowhere else; the
// unstranded forms stay in the tools' own units, which hold no other instantiation -- so a helper those kernels call has the one
// caller it always had, and the compiler makes of them what it made before.  The launches are all this unit gives.
#include "lsq_exonbins_dev.hpp"
#include "lsq_psi_count.hpp"
#include "lsq_evidence_count.hpp"

void lsq::xb_launch_stranded(unsigned grid, hipStream_t st, const ParsedReads &R, const XbIndex &I, unsigned long long *reads, unsigned long long *total, XbAcc *acc, unsigned lib_word, unsigned long long *lib) {
	hipLaunchKernelGGL((lsq_xb_count_kernel<true, unsigned, unsigned long long *>), dim3(grid), dim3(256), 0, st, R, I, reads, total, acc, lib_word, lib);
}

void lsq::ps_launch_stranded(unsigned grid, hipStream_t st, const ParsedReads &R, const PsIndex &I, unsigned min_overhang, unsigned long long *reads, unsigned long long *total, PsAcc *acc,
                             unsigned lib_word, unsigned long long *lib) {
	hipLaunchKernelGGL((lsq_ps_count_kernel<true, unsigned, unsigned long long *>), dim3(grid), dim3(256), 0, st, R, I, min_overhang, reads, total, acc, lib_word, lib);
}

void lsq::fe_launch_stranded(unsigned grid, hipStream_t st, const ParsedReads &R, const PsIndex &I, const FeIndex &F, unsigned min_overhang, unsigned min_body, unsigned long long *reads,
                             unsigned long long *total, FeAcc *acc, unsigned lib_word, unsigned long long *lib) {
	hipLaunchKernelGGL((lsq_fe_count_kernel<true, unsigned, unsigned long long *>), dim3(grid), dim3(256), 0, st, R, I, F, min_overhang, min_body, reads, total, acc, lib_word, lib);
}
