// Every executable: the reference's argv, stdout, stderr log and exit status (count/count.cpp:88-129, solve/solve.cpp:102-146,
// classify/classify.cpp:51-79), and the tools beside them.  The tool is chosen by the program name: the table of tools in
// lsq_cli.cpp names each with its function, and the Makefile's TOOLS the copies of this program.
#include "../../include/lesseq_hip.h"

int main(int argc, char **argv) {
	return lsq_cli_main(nullptr, argc, argv);
}
