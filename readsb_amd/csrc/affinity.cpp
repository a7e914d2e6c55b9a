// affinity.cpp — where the host side of a context runs: CPU affinity next to the device, and the device's pipeline slots.
#include "ctx.h"

// Put the host threads next to the device and next to each other: on the GPU's NUMA node (the
// record buffers are pinned host memory the GPU writes over PCIe, allocated there), and on
// physical cores that share one L3 — each stage reads what the previous one has just written, and a cross-CCD hand-off costs a fabric round trip per cache line.  The L3 group is
// picked by device ordinal so that the ranks of a node do not pile onto one CCD.
// MGPU_NO_AFFINITY=1 leaves the threads unbound.
static int sysfs_int(const std::string &path, int dflt) {
    FILE *f = fopen(path.c_str(), "r");
    if (!f) return dflt;
    int v = dflt;
    if (fscanf(f, "%d", &v) != 1) v = dflt;
    fclose(f);
    return v;
}

// Several contexts of one process on the same device (fan-in: one context per sample stream) must not pin their pipelines
// onto the same cores: the k-th live context of a device takes another L3 group (below).
static std::mutex g_slot_mu;
static uint32_t g_device_slots[64];          // bit k set = the device's k-th pipeline slot is taken

int take_device_slot(int device) {
    std::lock_guard<std::mutex> lk(g_slot_mu);
    uint32_t &m = g_device_slots[device & 63];
    for (int k = 0; k < 32; ++k)
        if (!(m & (1u << k))) { m |= 1u << k; return k; }
    return 0;
}

void release_device_slot(int device, int slot) {
    std::lock_guard<std::mutex> lk(g_slot_mu);
    g_device_slots[device & 63] &= ~(1u << slot);
}

// What the PROCESS may run on (cgroups, taskset): the mask of the thread that loaded the library, taken once, at load time.  Not the
// calling thread's mask of the moment: an application that follows mgpu_host_cpus' advice keeps its own threads — the one that
// creates the next context included — OFF the first context's cores, and a second context that picked its cores from that
// thread's mask landed on other L3 groups, its walk 2-3 x slower (bench.py's extra configurations, rounds 2 and 3).
static cpu_set_t g_process_cpus;
static bool g_process_cpus_ok = false;
__attribute__((constructor)) static void remember_process_cpus() { g_process_cpus_ok = sched_getaffinity(0, sizeof(g_process_cpus), &g_process_cpus) == 0; }
static bool process_cpus(cpu_set_t *out) {
    if (g_process_cpus_ok) { *out = g_process_cpus; return true; }
    return sched_getaffinity(0, sizeof(*out), out) == 0;
}

// CPUs of the device's NUMA node that the process may use (empty set: unknown)
static bool device_local_cpus(int device, cpu_set_t *out) {
    CPU_ZERO(out);
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, (int) sizeof(bus), device) != hipSuccess) return false;
    std::string id(bus);
    for (auto &ch : id) ch = (char) tolower((unsigned char) ch);
    FILE *f = fopen(("/sys/bus/pci/devices/" + id + "/local_cpulist").c_str(), "r");
    if (!f) return false;
    char line[4096] = {0};
    const bool ok = fgets(line, sizeof(line), f) != nullptr;
    fclose(f);
    if (!ok) return false;
    cpu_set_t allowed;
    if (!process_cpus(&allowed)) return false;
    int n = 0;
    for (char *tok = strtok(line, ",\n"); tok; tok = strtok(nullptr, ",\n")) {
        int a = 0, b = 0;
        const int got = sscanf(tok, "%d-%d", &a, &b);
        if (got == 1) b = a;
        if (got >= 1)
            for (int k = a; k <= b && k < CPU_SETSIZE; ++k)
                if (CPU_ISSET(k, &allowed)) { CPU_SET(k, out); ++n; }
    }
    return n > 0;
}

// Page-locked host memory is placed where the allocating thread runs: while the context allocates its buffers (the record
// copies' destinations, the counter blocks) the calling thread sits on the device's NUMA node, whatever CPU it came from —
// on a two-socket box a process that happened to start on the other socket had every pipeline stage read its records across
// the socket link (2.3 vs 2.6 ms per step from run to run).
NearDevice::NearDevice(int device) {
    if (getenv("MGPU_NO_AFFINITY")) return;
    cpu_set_t local;
    if (sched_getaffinity(0, sizeof(saved), &saved) != 0 || !device_local_cpus(device, &local)) return;
    moved = pthread_setaffinity_np(pthread_self(), sizeof(local), &local) == 0;
}
NearDevice::~NearDevice() { if (moved) (void) pthread_setaffinity_np(pthread_self(), sizeof(saved), &saved); }

static std::string sysfs_line(const std::string &path) {
    char line[4096] = {0};
    FILE *f = fopen(path.c_str(), "r");
    if (!f) return std::string();
    const bool ok = fgets(line, sizeof(line), f) != nullptr;
    fclose(f);
    std::string v = ok ? line : "";
    while (!v.empty() && (v.back() == '\n' || v.back() == ' ')) v.pop_back();
    return v;
}

// index of the PCI function `id` ("0000:c1:00.0") among the functions with its vendor, device id and local CPU list, ordered by address; -1: unknown
static int device_index_on_node(const std::string &id, const std::string &base = "/sys/bus/pci/devices/") {
    const std::string vendor = sysfs_line(base + id + "/vendor"), dev = sysfs_line(base + id + "/device"), cpus = sysfs_line(base + id + "/local_cpulist");
    if (vendor.empty() || dev.empty() || cpus.empty()) return -1;
    DIR *d = opendir(base.c_str());
    if (!d) return -1;
    std::vector<std::string> same;
    while (const dirent *e = readdir(d)) {
        const std::string name = e->d_name;
        if (name.empty() || name[0] == '.') continue;
        if (sysfs_line(base + name + "/vendor") == vendor && sysfs_line(base + name + "/device") == dev && sysfs_line(base + name + "/local_cpulist") == cpus)
            same.push_back(name);
    }
    closedir(d);
    std::sort(same.begin(), same.end());
    const auto it = std::find(same.begin(), same.end(), id);
    return it == same.end() ? -1 : (int) (it - same.begin());
}

// Two groups of threads, two L3 groups: `walk` (the walker and its helpers: they pass cache lines of the filter state and of
// the record list among themselves all the time) and `rest` (fetcher, builder and its helpers).  The hand-off between the
// two — one job per chunk — crosses CCDs once.  An 8-GPU node has two CCDs per GPU on the GPU's own NUMA node (EPYC 9575F:
// 16 L3 groups, 8 per socket, 4 GPUs per socket), so the first context of every device gets two groups of its own; further
// contexts of the same device (fan-in) put both groups of threads on one L3 group, half the node's groups away.
void bind_near_device(std::thread *const *walk, int nwalk, std::thread *const *rest, int nrest, int device, int device_slot,
                             std::vector<int> *pinned) {
    if (getenv("MGPU_NO_AFFINITY")) return;
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, (int) sizeof(bus), device) != hipSuccess) return;
    std::string id(bus);
    for (auto &ch : id) ch = (char) tolower((unsigned char) ch);
    FILE *f = fopen(("/sys/bus/pci/devices/" + id + "/local_cpulist").c_str(), "r");
    if (!f) return;
    char line[4096] = {0};
    const bool ok = fgets(line, sizeof(line), f) != nullptr;
    fclose(f);
    if (!ok) return;
    cpu_set_t allowed;                     // never step outside what the process may use (cgroups, taskset)
    if (!process_cpus(&allowed)) return;
    std::vector<int> cpus;
    for (char *tok = strtok(line, ",\n"); tok; tok = strtok(nullptr, ",\n")) {
        int a = 0, b = 0;
        const int got = sscanf(tok, "%d-%d", &a, &b);
        if (got == 1) b = a;
        if (got >= 1)
            for (int k = a; k <= b && k < CPU_SETSIZE; ++k)
                if (CPU_ISSET(k, &allowed)) cpus.push_back(k);
    }
    if (cpus.empty()) return;
    // L3 groups of the node, in first-appearance order
    std::vector<int> l3_ids, l3_of(cpus.size());
    for (size_t i = 0; i < cpus.size(); ++i) {
        l3_of[i] = sysfs_int("/sys/devices/system/cpu/cpu" + std::to_string(cpus[i]) + "/cache/index3/id", -1);
        if (std::find(l3_ids.begin(), l3_ids.end(), l3_of[i]) == l3_ids.end()) l3_ids.push_back(l3_of[i]);
    }
    // Which of the node's GPUs this is: its place among the PCI functions of the same vendor / device id on the same NUMA node, by bus
    // address (sysfs is not namespaced: a container that was handed ONE of a node's eight GPUs still sees the others there).  The HIP
    // ordinal is 0 in every such container — four of them on one socket picked the same two L3 groups and the same cores (round 5:
    // now and then a benchmark process ran at 0.6 of the rate with one host stage slow and nothing else changed).  Ranks that
    // share one device (tests) or see one device each (per-rank HIP_VISIBLE_DEVICES) still spread out by LOCAL_RANK.
    int ordinal = device_index_on_node(id);
    if (ordinal < 0) ordinal = device;
    if (const char *lr = getenv("LOCAL_RANK")) { const int v = atoi(lr); if (v >= 0) ordinal = v; }
    const size_t ng = l3_ids.size();
    int want_walk, want_rest;
    if (device_slot == 0 && ng >= 2) {
        want_walk = l3_ids[((size_t) ordinal * 2) % ng];
        want_rest = l3_ids[((size_t) ordinal * 2 + 1) % ng];
    } else {   // further contexts of the same device: half the node's groups away, where an 8-GPU node's other devices do not sit
        const size_t stride = ng >= 2 ? ng / 2 : 1;
        want_walk = want_rest = l3_ids[((size_t) ordinal * 2 + (size_t) device_slot * stride + (size_t) (device_slot / 2)) % ng];
    }
    // one logical CPU per physical core of a group; more threads than cores share cores round-robin
    auto cores_of = [&](int want) {
        std::vector<int> pick, cores;
        for (size_t i = 0; i < cpus.size(); ++i) {
            if (l3_of[i] != want) continue;
            const int core = sysfs_int("/sys/devices/system/cpu/cpu" + std::to_string(cpus[i]) + "/topology/core_id", (int) i);
            if (std::find(cores.begin(), cores.end(), core) != cores.end()) continue;
            cores.push_back(core);
            pick.push_back(cpus[i]);
        }
        return pick;
    };
    const std::vector<int> pw = cores_of(want_walk), pr = cores_of(want_rest);
    cpu_set_t set;
    if (want_walk >= 0 && pw.size() >= 2 && pr.size() >= 2) {
        const bool same = want_walk == want_rest;
        for (int t = 0; t < nwalk; ++t) {
            CPU_ZERO(&set); CPU_SET(pw[(size_t) t % pw.size()], &set);
            (void) pthread_setaffinity_np(walk[t]->native_handle(), sizeof(set), &set);
        }
        for (int t = 0; t < nrest; ++t) {       // on a shared group the second set of threads continues where the first ended
            CPU_ZERO(&set); CPU_SET(pr[(size_t) (t + (same ? nwalk : 0)) % pr.size()], &set);
            (void) pthread_setaffinity_np(rest[t]->native_handle(), sizeof(set), &set);
        }
        if (pinned) {
            pinned->clear();
            for (int t = 0; t < nwalk && t < (int) pw.size(); ++t) pinned->push_back(pw[(size_t) t]);
            for (int t = 0; t < nrest && t < (int) pr.size(); ++t) {
                const int cpu = pr[(size_t) (t + (same ? nwalk : 0)) % pr.size()];
                if (std::find(pinned->begin(), pinned->end(), cpu) == pinned->end()) pinned->push_back(cpu);
            }
        }
    } else {                               // no cache topology in sysfs: the whole node
        CPU_ZERO(&set);
        for (int k : cpus) CPU_SET(k, &set);
        for (int t = 0; t < nwalk; ++t) (void) pthread_setaffinity_np(walk[t]->native_handle(), sizeof(set), &set);
        for (int t = 0; t < nrest; ++t) (void) pthread_setaffinity_np(rest[t]->native_handle(), sizeof(set), &set);
    }
}

extern "C" {

int mgpu_selftest_device_index(const char *pci_devices_dir, const char *bus_id) {
    if (!pci_devices_dir || !bus_id) return -2;
    std::string base(pci_devices_dir);
    if (base.empty() || base.back() != '/') base += '/';
    return device_index_on_node(bus_id, base);
}

int mgpu_host_cpus(mgpu_ctx *c, int32_t *cpus, int32_t cap) {
    if (!c || (!cpus && cap)) return MGPU_E_INVAL;
    const int n = (int) c->host_cpus.size();
    for (int i = 0; i < n && i < cap; ++i) cpus[i] = c->host_cpus[i];
    return n;
}

}  // extern "C"
