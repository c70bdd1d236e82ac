package main

import (
	"encoding/json"
	"errors"
	"fmt"
	"log"
	"math"
	"net/http"
	"reflect"
	"sort"
	"sync"

	"gorilla-rag/vsearch"
)

type service struct {
	eng    *vsearch.Engine
	dim    uint32
	dtype  int
	mu     sync.RWMutex
	stores map[string]*pointStore
	order  []string
	batch  *batcher
}

func newService(eng *vsearch.Engine, dim uint32, dtype int) *service {
	return &service{eng: eng, dim: dim, dtype: dtype, stores: map[string]*pointStore{},
		batch: newBatcher(eng, dim)}
}

// initCollections: Get, and Create on NotFound (main.go:80-119).
func (s *service) initCollections(names []string) error {
	for _, name := range names {
		_, rows, err := s.eng.Info(name)
		if errors.Is(err, vsearch.ErrNotFound) {
			log.Printf("Creating collection: %s", name)
			err = s.eng.Create(name, s.dim, vsearch.MetricCosine, s.dtype, 0)
		} else if err == nil && rows != 0 {
			err = fmt.Errorf("collection %s holds %d rows without point ids", name, rows)
		}
		if err != nil {
			return fmt.Errorf("failed to create collection %s: %w", name, err)
		}
		s.mu.Lock()
		s.stores[name] = newPointStore()
		s.order = append(s.order, name)
		s.mu.Unlock()
	}
	return nil
}

func (s *service) store(name string) *pointStore {
	s.mu.RLock()
	defer s.mu.RUnlock()
	return s.stores[name]
}

// restore loads <dir>/<coll>.vsnap (rows) and <coll>.points.json (ids,
// payloads) into the still empty collections.
func (s *service) restore(dir string) error {
	for _, name := range s.order {
		st := s.store(name)
		if err := s.eng.Drop(name); err != nil {
			return err
		}
		if err := s.eng.Restore(name, rowsPath(dir, name)); err != nil {
			_ = s.eng.Create(name, s.dim, vsearch.MetricCosine, s.dtype, 0)
			return err
		}
		if err := st.load(sidecarPath(dir, name)); err != nil {
			_ = s.eng.Drop(name)
			_ = s.eng.Create(name, s.dim, vsearch.MetricCosine, s.dtype, 0)
			return err
		}
		if _, rows, err := s.eng.Info(name); err != nil || rows != uint64(len(st.ids)) {
			return fmt.Errorf("restore %s: %d rows for %d point ids", name, rows, len(st.ids))
		}
	}
	return nil
}

func writeJSON(w http.ResponseWriter, status int, v interface{}) {
	w.Header().Set("Content-Type", "application/json")
	w.WriteHeader(status)
	_ = json.NewEncoder(w).Encode(v) // HTML-escaped, "\n"-terminated, as the reference's
}

func writeError(w http.ResponseWriter, status int, msg string) {
	writeJSON(w, status, map[string]string{"error": msg})
}

func (s *service) health(w http.ResponseWriter, r *http.Request) {
	info, err := s.eng.Health()
	out := map[string]string{"service": "vector-service", "status": "healthy"}
	if err != nil {
		out["status"] = "degraded"
		out["error"] = err.Error()
	} else {
		var h struct {
			DeviceName string `json:"device_name"`
		}
		_ = json.Unmarshal([]byte(info), &h)
		out["engine"] = "vsearch-hip " + h.DeviceName
	}
	writeJSON(w, http.StatusOK, out)
}

func (s *service) collections(w http.ResponseWriter, r *http.Request) {
	if r.Method != http.MethodGet {
		http.Error(w, "Method not allowed", http.StatusMethodNotAllowed)
		return
	}
	writeJSON(w, http.StatusOK, map[string][]string{"collections": collectionNames})
}

type upsertBody struct {
	Collection string                   `json:"collection"`
	Points     []map[string]interface{} `json:"points"`
}

// toFloat32 converts a decoded JSON array ([]interface{} of float64) the way
// the reference's convertVector does (main.go:343-375): float32(x) per element.
func toFloat32(v interface{}) ([]float32, error) {
	arr, ok := v.([]interface{})
	if !ok {
		return nil, errors.New("point vector must be an array")
	}
	out := make([]float32, len(arr))
	for i, x := range arr {
		f, ok := x.(float64)
		if !ok {
			return nil, errors.New("vector contains non-numeric value")
		}
		out[i] = float32(f)
	}
	return out, nil
}

func (s *service) upsert(w http.ResponseWriter, r *http.Request) {
	if r.Method != http.MethodPost {
		http.Error(w, "Method not allowed", http.StatusMethodNotAllowed)
		return
	}
	var body upsertBody
	if err := json.NewDecoder(r.Body).Decode(&body); err != nil {
		writeError(w, http.StatusBadRequest, "Invalid request body")
		return
	}
	if body.Collection == "" {
		writeError(w, http.StatusBadRequest, "Collection name required")
		return
	}
	log.Printf("Upserting %d points to collection: %s", len(body.Points), body.Collection)
	n := len(body.Points)
	ids := make([]string, n)
	vecs := make([][]float32, n)
	payloads := make([]map[string]interface{}, n)
	for i, p := range body.Points {
		id, ok := p["id"].(string)
		if !ok {
			writeError(w, http.StatusBadRequest, "Point ID must be a string")
			return
		}
		raw, ok := p["vector"]
		if !ok {
			writeError(w, http.StatusBadRequest, "Point vector must be provided")
			return
		}
		v, err := toFloat32(raw)
		if err != nil {
			writeError(w, http.StatusBadRequest, err.Error())
			return
		}
		ids[i], vecs[i] = id, v
		if pl, ok := p["payload"].(map[string]interface{}); ok {
			payloads[i] = pl
		}
	}
	st := s.store(body.Collection)
	if st == nil {
		writeError(w, http.StatusInternalServerError, "Failed to upsert: collection "+
			body.Collection+" not found")
		return
	}
	for i := range ids {
		c, ok := canonicalUUID(ids[i])
		if !ok {
			writeError(w, http.StatusInternalServerError, "Failed to upsert: Unable to parse UUID: "+ids[i])
			return
		}
		ids[i] = c
		if uint32(len(vecs[i])) != s.dim {
			writeError(w, http.StatusInternalServerError, fmt.Sprintf(
				"Failed to upsert: Vector dimension error: expected dim: %d, got %d", s.dim, len(vecs[i])))
			return
		}
	}
	flat := make([]float32, 0, n*int(s.dim))
	for _, v := range vecs {
		flat = append(flat, v...)
	}
	st.mu.Lock()
	rows, total := st.assign(ids)
	if err := s.eng.Upsert(body.Collection, s.dim, rows, flat); err != nil {
		st.mu.Unlock()
		writeError(w, http.StatusInternalServerError, "Failed to upsert: "+err.Error())
		return
	}
	st.commit(ids, rows, payloads, total)
	st.mu.Unlock()
	writeJSON(w, http.StatusOK, map[string]interface{}{
		"status": "success", "collection": body.Collection, "points": n})
}

type deleteBody struct {
	Collection string                 `json:"collection"`
	IDs        []interface{}          `json:"ids"`
	Filter     map[string]interface{} `json:"filter"`
}

// remove serves POST /delete, an extension outside the reference's four
// routes (Qdrant's Points.Delete has no call site there): the points named by
// "ids", or those whose payload holds every "filter" key with an equal value,
// go through Engine.Delete, and the store is renumbered from the moves under
// the collection's writer lock (search holds the reader lock through its
// decode, so an answer belongs to one version). Unknown ids are ignored.
func (s *service) remove(w http.ResponseWriter, r *http.Request) {
	if r.Method != http.MethodPost {
		http.Error(w, "Method not allowed", http.StatusMethodNotAllowed)
		return
	}
	var body deleteBody
	if err := json.NewDecoder(r.Body).Decode(&body); err != nil {
		writeError(w, http.StatusBadRequest, "Invalid request body")
		return
	}
	if body.Collection == "" {
		writeError(w, http.StatusBadRequest, "Collection name required")
		return
	}
	if (body.IDs != nil) == (body.Filter != nil) {
		writeError(w, http.StatusBadRequest, "Exactly one of ids and filter must be given")
		return
	}
	if body.Filter != nil && len(body.Filter) == 0 { // it would match every point
		writeError(w, http.StatusBadRequest, "filter must not be empty")
		return
	}
	ids := make([]string, len(body.IDs))
	for i, v := range body.IDs {
		id, ok := v.(string)
		if !ok {
			writeError(w, http.StatusBadRequest, "Point ID must be a string")
			return
		}
		ids[i] = id
	}
	st := s.store(body.Collection)
	if st == nil {
		writeError(w, http.StatusInternalServerError, "Failed to delete: collection "+
			body.Collection+" not found")
		return
	}
	for i := range ids {
		c, ok := canonicalUUID(ids[i])
		if !ok {
			writeError(w, http.StatusInternalServerError, "Failed to delete: Unable to parse UUID: "+ids[i])
			return
		}
		ids[i] = c
	}
	st.mu.Lock()
	defer st.mu.Unlock()
	var rows []uint64
	if body.IDs != nil {
		seen := map[uint64]bool{}
		for _, id := range ids {
			if row, ok := st.rowOf[id]; ok && !seen[row] {
				seen[row] = true
				rows = append(rows, row)
			}
		}
		sort.Slice(rows, func(a, b int) bool { return rows[a] < rows[b] })
	} else {
		for row, pl := range st.payloads {
			match := true
			for k, v := range body.Filter {
				if got, ok := pl[k]; !ok || !reflect.DeepEqual(got, v) {
					match = false
					break
				}
			}
			if match {
				rows = append(rows, uint64(row))
			}
		}
	}
	if len(rows) > 0 {
		from, to, err := s.eng.Delete(body.Collection, rows)
		if err != nil {
			msg := "Failed to delete: " + err.Error()
			// the engine compacted the rows but the moves were lost: the ids here no
			// longer match its rows, so the collection is emptied on both sides
			if _, now, ierr := s.eng.Info(body.Collection); ierr == nil && now != uint64(len(st.ids)) {
				_ = s.eng.Drop(body.Collection)
				_ = s.eng.Create(body.Collection, s.dim, vsearch.MetricCosine, s.dtype, 0)
				st.rowOf, st.ids, st.payloads = map[string]uint64{}, nil, nil
				msg += " (the collection was emptied)"
			}
			writeError(w, http.StatusInternalServerError, msg)
			return
		}
		st.remove(rows, from, to)
	}
	writeJSON(w, http.StatusOK, map[string]interface{}{
		"status": "success", "collection": body.Collection, "deleted": len(rows)})
}

type searchBody struct {
	Collection string                 `json:"collection"`
	Query      []float32              `json:"query"` // decimal -> float32 directly, as main.go:28
	TopK       int                    `json:"top_k"`
	Filter     map[string]interface{} `json:"filter"` // accepted, not applied (main.go:30)
	MMR        *mmrBody               `json:"mmr"`    // an extension: Qdrant's query-API mmr object
	// an extension: Qdrant's SearchGroups (include/vsearch_service.h)
	GroupBy   *string `json:"group_by"`
	GroupSize *int    `json:"group_size"` // default 1: the best chunk per document
	Fusion    *fusionBody `json:"fusion"` // an extension: Qdrant's query-API prefetch + fusion
}

// fusionBody is /search's optional "fusion" object (include/vsearch_service.h):
// the request's own query is sub-query 0 and Queries holds 1 to 7 more vectors
// (decoded loosely: toFloat32 applies convertVector's rules to each); Method
// defaults to "rrf", PrefetchLimit to 0 (the engine's min(4 top_k, 128)) and
// RRFK to 0 (the engine's 2; not allowed with "dbsf").
type fusionBody struct {
	Method        *string       `json:"method"`
	Queries       []interface{} `json:"queries"`
	PrefetchLimit *int          `json:"prefetch_limit"`
	RRFK          *int          `json:"rrf_k"`
}

// mmrBody is /search's optional "mmr" object (include/vsearch_service.h): both
// fields optional, defaults 0.5 and 0 (the engine's min(4 top_k, 128)).
type mmrBody struct {
	Diversity       *float64 `json:"diversity"`
	CandidatesLimit *int     `json:"candidates_limit"`
}

type hit struct {
	ID      string                 `json:"id"`
	Score   float64                `json:"score"`
	Payload map[string]interface{} `json:"payload"`
}

type searchReply struct {
	Results []hit `json:"results"`
	Count   int   `json:"count"`
}

// groupedReply is /search's reply with "group_by": results flat in group
// order (a group's hits adjacent), groups in the same order.
type groupedReply struct {
	Results []hit       `json:"results"`
	Count   int         `json:"count"`
	Groups  []groupInfo `json:"groups"`
}

type groupInfo struct {
	ID   interface{} `json:"id"` // the payload value, as given
	Hits int         `json:"hits"`
}

// groupKey is the group of a payload value: strings and integers are groups
// (Qdrant's keyword and integer group keys), anything else is none.
func groupKey(v interface{}) (string, bool) {
	switch x := v.(type) {
	case string:
		return "s" + x, true
	case float64: // encoding/json's number
		if x == math.Trunc(x) && math.Abs(x) < 1<<63 {
			return fmt.Sprintf("i%d", int64(x)), true
		}
	}
	return "", false
}

// groupingFor returns the store's current grouping by payload key `key`,
// building it (and letting stale ones go) when needed. Reader lock held.
func (s *service) groupingFor(coll string, st *pointStore, key string) (*grouping, error) {
	st.gmu.Lock()
	defer st.gmu.Unlock()
	if g, ok := st.groupings[key]; ok && g.version == st.version {
		return g, nil
	}
	for k, g := range st.groupings { // stale ones serve nobody: searches hold the reader lock
		if g.version != st.version {
			_ = s.eng.GroupingDrop(g.id) // gone already after a delete
			delete(st.groupings, k)
		}
	}
	g := &grouping{version: st.version}
	dense := map[string]uint32{}
	gor := make([]uint32, len(st.payloads))
	for r, pl := range st.payloads {
		gor[r] = vsearch.GroupNone
		if v, ok := pl[key]; ok {
			if k, ok := groupKey(v); ok {
				id, seen := dense[k]
				if !seen {
					id = uint32(len(g.values))
					dense[k] = id
					g.values = append(g.values, v)
				}
				gor[r] = id
			}
		}
	}
	id, err := s.eng.GroupingCreate(coll, gor, uint32(len(g.values)))
	if err != nil {
		return nil, err
	}
	g.id = id
	if st.groupings == nil {
		st.groupings = map[string]*grouping{}
	}
	st.groupings[key] = g
	return g, nil
}

func (s *service) search(w http.ResponseWriter, r *http.Request) {
	if r.Method != http.MethodPost {
		http.Error(w, "Method not allowed", http.StatusMethodNotAllowed)
		return
	}
	var body searchBody
	if err := json.NewDecoder(r.Body).Decode(&body); err != nil {
		writeError(w, http.StatusBadRequest, "Invalid request body")
		return
	}
	if body.TopK == 0 {
		body.TopK = 5
	}
	if body.TopK < 0 {
		writeError(w, http.StatusBadRequest, "top_k must not be negative")
		return
	}
	diversity, candidates := float32(0.5), uint32(0)
	if m := body.MMR; m != nil {
		if m.Diversity != nil {
			if !(*m.Diversity >= 0 && *m.Diversity <= 1) {
				writeError(w, http.StatusBadRequest, "Invalid request body")
				return
			}
			diversity = float32(*m.Diversity)
		}
		if m.CandidatesLimit != nil {
			if *m.CandidatesLimit < 0 || *m.CandidatesLimit > int(vsearch.MMRMaxCandidates) {
				writeError(w, http.StatusBadRequest, "Invalid request body")
				return
			}
			candidates = uint32(*m.CandidatesLimit)
		}
	}
	groupSize := 1
	if body.GroupSize != nil {
		if *body.GroupSize < 1 || *body.GroupSize > int(vsearch.GroupsMaxSize) {
			writeError(w, http.StatusBadRequest, "Invalid request body")
			return
		}
		groupSize = *body.GroupSize
	}
	if body.GroupBy != nil && body.MMR != nil {
		writeError(w, http.StatusBadRequest, "Invalid request body")
		return
	}
	fusion, prefetch, rrfK := vsearch.FusionRRF, uint32(0), uint32(0)
	var subs [][]float32 // fusion.queries, converted
	if f := body.Fusion; f != nil {
		if f.Method != nil {
			switch *f.Method {
			case "rrf":
			case "dbsf":
				fusion = vsearch.FusionDBSF
			default:
				writeError(w, http.StatusBadRequest, "Invalid request body")
				return
			}
		}
		bad := len(f.Queries) == 0 || len(f.Queries) > int(vsearch.FuseMaxLists)-1 ||
			(f.PrefetchLimit != nil && (*f.PrefetchLimit < 0 || *f.PrefetchLimit > int(vsearch.FuseMaxLimit))) ||
			(f.RRFK != nil && (*f.RRFK < 0 || *f.RRFK > 65536 || fusion == vsearch.FusionDBSF)) ||
			body.MMR != nil || body.GroupBy != nil
		if bad {
			writeError(w, http.StatusBadRequest, "Invalid request body")
			return
		}
		if f.PrefetchLimit != nil {
			prefetch = uint32(*f.PrefetchLimit)
		}
		if f.RRFK != nil {
			rrfK = uint32(*f.RRFK)
		}
		for _, q := range f.Queries {
			v, err := toFloat32(q)
			if err != nil {
				writeError(w, http.StatusBadRequest, err.Error())
				return
			}
			subs = append(subs, v)
		}
	}
	log.Printf("Searching in collection: %s, TopK: %d", body.Collection, body.TopK)
	st := s.store(body.Collection)
	if st == nil {
		writeError(w, http.StatusInternalServerError, "Search failed: collection "+
			body.Collection+" not found")
		return
	}
	st.mu.RLock()
	defer st.mu.RUnlock()
	if uint32(len(body.Query)) != s.dim {
		writeError(w, http.StatusInternalServerError, fmt.Sprintf(
			"Search failed: Vector dimension error: expected dim: %d, got %d", s.dim, len(body.Query)))
		return
	}
	for _, v := range subs {
		if uint32(len(v)) != s.dim {
			writeError(w, http.StatusInternalServerError, fmt.Sprintf(
				"Search failed: Vector dimension error: expected dim: %d, got %d", s.dim, len(v)))
			return
		}
	}
	if body.GroupBy != nil {
		s.searchGroups(w, &body, st, groupSize)
		return
	}
	reply := searchReply{Results: make([]hit, 0)}
	if rows := len(st.ids); rows > 0 {
		k := body.TopK
		if k > rows { // Qdrant returns min(limit, points); any limit is served
			k = rows
		}
		hits, err := vsearch.Hits{}, error(nil)
		if body.Fusion != nil {
			// one engine call per request, past the batcher: query and fusion.queries
			// are the sub-queries of one fused query; scores are the fused scores
			if k > int(vsearch.FuseMaxLimit) {
				writeError(w, http.StatusBadRequest, fmt.Sprintf(
					"top_k must not exceed %d with fusion", vsearch.FuseMaxLimit))
				return
			}
			if prefetch != 0 && prefetch < uint32(k) {
				prefetch = uint32(k)
			}
			all := append([]float32{}, body.Query...)
			for _, v := range subs {
				all = append(all, v...)
			}
			var hs []vsearch.Hits
			hs, err = s.eng.SearchFused(body.Collection, all, uint32(1+len(subs)), s.dim, uint32(k),
				prefetch, fusion, rrfK, 0)
			if err == nil {
				hits = hs[0]
			}
		} else if body.MMR != nil {
			// one engine call per request, past the batcher; results in selection order
			if k > int(vsearch.MMRMaxCandidates) {
				writeError(w, http.StatusBadRequest, fmt.Sprintf(
					"top_k must not exceed %d with mmr", vsearch.MMRMaxCandidates))
				return
			}
			if candidates != 0 && candidates < uint32(k) {
				candidates = uint32(k)
			}
			var hs []vsearch.Hits
			hs, err = s.eng.SearchMMR(body.Collection, body.Query, s.dim, uint32(k), candidates,
				diversity, 0)
			if err == nil {
				hits = hs[0]
			}
		} else {
			hits, err = s.batch.search(body.Collection, body.Query, uint32(k))
		}
		if err != nil {
			writeError(w, http.StatusInternalServerError, "Search failed: "+err.Error())
			return
		}
		for i, row := range hits.Rows {
			pl := st.payloads[row]
			if pl == nil {
				pl = map[string]interface{}{}
			}
			reply.Results = append(reply.Results, hit{ID: st.ids[row],
				Score: float64(hits.Scores[i]), Payload: pl})
		}
	}
	reply.Count = len(reply.Results)
	writeJSON(w, http.StatusOK, reply)
}

// searchGroups answers a /search carrying "group_by": one SearchGroups call
// per request, past the batcher. The store's reader lock is held.
func (s *service) searchGroups(w http.ResponseWriter, body *searchBody, st *pointStore,
	groupSize int) {
	reply := groupedReply{Results: make([]hit, 0), Groups: make([]groupInfo, 0)}
	k := body.TopK
	if rows := len(st.ids); k > rows && rows > 0 {
		k = rows
	}
	if k > int(vsearch.GroupsMaxLimit) {
		writeError(w, http.StatusBadRequest, fmt.Sprintf(
			"top_k must not exceed %d with group_by", vsearch.GroupsMaxLimit))
		return
	}
	if len(st.ids) > 0 {
		g, err := s.groupingFor(body.Collection, st, *body.GroupBy)
		if err != nil {
			writeError(w, http.StatusInternalServerError, "Search failed: "+err.Error())
			return
		}
		res, err := s.eng.SearchGroups(body.Collection, body.Query, s.dim, uint32(k),
			uint32(groupSize), g.id, 0)
		if err != nil {
			writeError(w, http.StatusInternalServerError, "Search failed: "+err.Error())
			return
		}
		for _, grp := range res[0] {
			for i, row := range grp.Hits.Rows {
				pl := st.payloads[row]
				if pl == nil {
					pl = map[string]interface{}{}
				}
				reply.Results = append(reply.Results, hit{ID: st.ids[row],
					Score: float64(grp.Hits.Scores[i]), Payload: pl})
			}
			reply.Groups = append(reply.Groups, groupInfo{ID: g.values[grp.ID],
				Hits: len(grp.Hits.Rows)})
		}
	}
	reply.Count = len(reply.Results)
	writeJSON(w, http.StatusOK, reply)
}
