function [pk,vk,ak,K_T_used,scene_status,waypoints,n_wp,replan_count,replan_col,wp_col,plan_status] = replanRoutes(po,goals,prm,K_T_max,error_tol,cell,capture,margin,W,every,ahead,path,timeout)
% Re-planned routes (no reference counterpart): planRoutes before column 0, the flight of dmpc_mex('route', ..) from there, and every `every` columns
% (default 5, 0 = never) the agents whose remaining legs are no longer clear are planned again on the device, from where they are, round the
% vehicles where they are on that column and on the `ahead` (default 0) columns behind it.
% po: 3 x N (or 1 x 3 x N); goals: 3 x N_cmd.  path (3 x P x M, optional): scripted vehicles, path(:,t+1,j) is vehicle j on column t (the last
% sample stays); po is then 3 x N_cmd.  Without a path the vehicles of po behind the commanded ones are static obstacles.
% prm: a dmpc_params_struct.  cell, margin (default 0), W (default 4): planRoutes'; capture (metres), timeout (columns, default 0 = none): 'route''s.
% pk, vk, ak (3 x K_T_max x N_cmd), K_T_used, scene_status: as 'transition'.  waypoints (3 x W x N_cmd), n_wp, plan_status (1 x N_cmd): the plan in
% force when the trial ended; wp_col (W x N_cmd) refers to it.  replan_count, replan_col (1 x N_cmd): the re-plans of every agent and the 0-based
% column of its last one, -1 for none.
po = reshape(po,3,[]); goals = reshape(goals,3,[]);
if nargin < 8, margin = []; end
if nargin < 9, W = []; end
if nargin < 10, every = []; end
if nargin < 11, ahead = []; end
if nargin < 12, path = []; end
if nargin < 13, timeout = []; end
[pk,vk,ak,K_T_used,scene_status,waypoints,n_wp,replan_count,replan_col,wp_col,plan_status] = dmpc_mex('replan', prm, po, goals, K_T_max, error_tol, cell, capture, margin, W, every, ahead, path, timeout);
end
