// breakdancer-max: same command line, configuration format and output columns as the reference
// (exe/breakdancer-max/BreakDancerMax.cpp:38-163); the clustering path runs on the GPU through libbdx.
#include <cerrno>
#include <csignal>
#include <cstdio>
#include <exception>
#include <iostream>
#include <time.h>

#include <fcntl.h>
#include <sys/prctl.h>
#include <sys/wait.h>
#include <unistd.h>

#include "bdx.h"
#include "inputs.h"
#include "phases.h"
#include "table.h"

using namespace bdhost;

namespace {

// The command's result is complete (everything printed, the dump files closed): tell the process that was started, which returns
// at once; this one -- which owns the GPU context -- goes on to hand gigabytes of HBM and the pinned buffers back to the driver
// (~0.1 s for a chromosome), with its standard streams closed so that a reader of the pipe sees the end of the output now.
int g_report_fd = -1;
void report_result(int status) {
    std::cout.flush();
    fflush(nullptr);
    if (g_report_fd < 0) return;
    const ssize_t w = write(g_report_fd, &status, sizeof status);
    (void)w;
    close(g_report_fd);
    g_report_fd = -1;
    close(STDOUT_FILENO);
    close(STDERR_FILENO);
}

void print_wall_clock(const char* what) {
    struct timespec ts;
    clock_gettime(CLOCK_REALTIME, &ts);
    fprintf(stderr, "[bdx timing] %s at %.6f (wall clock)\n", what, (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec);
}

// Everything is printed: the process ends here.  Releasing tens of buffers, the pinned pages and the HIP runtime one by one
// takes longer than the whole GPU path ran (0.03-0.05 s for a chromosome); the operating system does it in one go.
// BDX_CLEAN_EXIT=1 returns instead and walks the destructors, the session's among them (leak checkers).
void leave(const Inputs& in, const Env& env, const Session& s, Support& sup) {
    if (env.clean_exit) return;
    sup.bed.reset();     // (the dump files are closed by their writers' destructors)
    sup.fastq.reset();
    // (but not with work still queued on a device -- a record stage of the decoder's last batch, a copy nobody waits for: the
    // driver then takes 0.11-0.16 s to tear the queues down, against 0.015 s for an idle device.  bdx_warm_up ends in a device-wide wait)
    if (in.sharded) { for (int dv : in.devices) (void)bdx_warm_up(dv); }
    else (void)bdx_warm_up(bdx_device(s.ctx));
    report_result(0);
    if (env.timing) print_wall_clock("_exit called");
    _exit(0);
}

int run(int argc, char** argv, const Env& env) {
    Session s;   // (outside the try: whatever ends the run, the session goes behind it, in its destructor's one order)
    try {
        Inputs in(argc, argv, env);   // (--estimate replaces its libraries between "fed" and "run": Inputs::apply_estimate)
        if (in.no_bams) {
            std::cout << "Error: no bams files in config file!\n";
            return 1;
        }
        const auto t_start = Clock::now();
        const Fed fed = in.sharded ? feed_and_run_sharded(in, env, s, t_start) : feed_and_run_single(in, env, s, t_start);
        const Statistics st = fetch_statistics(in, s);
        if (!in.opts.cache_file.empty()) write_pass1_cache(in, st);
        const TableFormat table(in.opts, in.cfg, fed.targets);
        table.header(std::cout, st.counters);
        const Calls calls = fetch_calls(s, st.sum.n_svs);
        // (--vcf: the junction counts run before the trimmer starts, which must not run beside another call on the context)
        Genotypes gt = count_on_store(in, env, s, fed, calls);
        call_mini(in, env, s, fed);
        call_anchor(in, env, s, fed);
        // (a large run's pinned result tables go back while the table is printed: the process's end is that much shorter.  BDX_TRIM=0: kept)
        if (fed.n_reads > (size_t)(8u << 20) && !in.want_dumps && !env.clean_exit && !env.keep_results) s.start_trimmer();
        Support sup = fetch_support(in, s, fed, calls);
        write_table(in, env, table, calls, sup);
        write_vcfs(in, gt);
        if (env.timing) print_timing(in, s, fed, st, t_start);
        leave(in, env, s, sup);
    } catch (std::exception const& e) {
        std::cerr << "ERROR: " << e.what() << "\n";
        return 1;
    }
    return 0;
}

}  // namespace

// Releasing a GPU context takes the driver longer than the whole GPU path runs, and a process cannot return before its resources
// are gone.  So the work is done by a child (forked before the HIP runtime is touched); the process the user started waits for the
// child's word that the table is written and returns with its status, while the child's exit takes its time in the background.
// BDX_FOREGROUND=1 (and BDX_CLEAN_EXIT=1, the leak checkers' mode) keep everything in the one process.
int main(int argc, char** argv) {
    const Env env = read_env();
    if (env.timing) print_wall_clock("main() entered");   // (for whoever times the process from outside: when main() was reached)
    if (!env.foreground && !env.clean_exit) {
        int pfd[2];
        if (pipe(pfd) == 0) {
            const pid_t parent = getpid();   // (may be 1: a container's entry point)
            const pid_t pid = fork();
            if (pid > 0) {
                close(pfd[1]);
                int status = 1;
                ssize_t r;
                do r = read(pfd[0], &status, sizeof status); while (r < 0 && errno == EINTR);
                if (r == (ssize_t)sizeof status) _exit(status);
                int ws = 0;   // the child ended without reporting: usage errors (exit inside the option parser), crashes
                while (waitpid(pid, &ws, 0) < 0 && errno == EINTR) {}
                if (WIFEXITED(ws)) _exit(WEXITSTATUS(ws));
                if (WIFSIGNALED(ws)) { signal(WTERMSIG(ws), SIG_DFL); raise(WTERMSIG(ws)); }
                _exit(1);
            }
            if (pid == 0) {
                close(pfd[0]);
                g_report_fd = pfd[1];
                fcntl(g_report_fd, F_SETFD, FD_CLOEXEC);
                // (killing the command kills the work: the child is told when the process that was started goes -- after the report
                // that only cuts its exit short)
                prctl(PR_SET_PDEATHSIG, SIGTERM);
                if (getppid() != parent) _exit(1);   // (the parent went before the signal was armed)
            } else {  // (no child: everything in this process)
                close(pfd[0]);
                close(pfd[1]);
            }
        }
    }
    const int rc = run(argc, argv, env);
    report_result(rc);
    return rc;
}
